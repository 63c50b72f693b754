"""The carried pitch path of include/tinyvc_hip.h restated in numpy fp32, on helpers_pitch_path's own pieces (emission, cost_matrix,
_normalise, _walk_back): the full 512 x 512 form of the definition with a sanitised prior in front of frame 0 and the best-predecessor
values of frame `carry_frame` taken on the way.  Every arithmetic step is one correctly rounded fp32 operation, as there.

The prefix property the feature rests on: decoded window by window over slices of ONE logits tensor - window n = frames [n h, n h + T), its
prior the carry of window n - 1 - scores, back-pointers and path equal helpers_pitch_path's decode of the whole prefix [0, n h + T), by
value: the carry of window n - 1 is best_{n h} of the prefix, so u_0 of window n is u_{n h} of the prefix, and nothing later looks further
back than s_{t-1}."""
import numpy as np

import helpers_pitch_path as H

F = H.F


def sanitise(prior):
    """the prior as the recursion takes it: values <= 0 (-inf included) as they are, everything else - NaN, positive values, +inf - 0; a state
    that is -inf throughout after that is zeros (a reset)"""
    p = np.asarray(prior, dtype=F)
    with np.errstate(invalid="ignore"):
        p = np.where(p <= 0, p, F(0)).astype(F)
    return np.zeros_like(p) if np.isneginf(p).all() else p


def viterbi_carried(logits, s, prior=None, carry_frame=0):
    """-> (path [T] int32, bp [T, 512] (row 0 unused), s_{T-1} [512] fp32, carry [512] fp32 = best_h for h = carry_frame >= 1, else None).
    prior None is helpers_pitch_path.viterbi_full."""
    e = H.emission(logits)
    T = e.shape[1]
    assert carry_frame == 0 or 1 <= carry_frame < T, "frame h must exist"
    cost = H.cost_matrix(s)
    bp = np.zeros((T, H.CLASSES), np.int32)
    carry = None
    with np.errstate(invalid="ignore", over="ignore"):
        u0 = e[:, 0] if prior is None else (sanitise(prior) + e[:, 0]).astype(F)
        sc = H._normalise(u0)
        for t in range(1, T):
            cand = (sc[:, None] - cost).astype(F)      # cand[i, j]
            bp[t] = np.argmax(cand, axis=0)            # the lowest i on equal values
            best = cand.max(axis=0)
            if t == carry_frame:
                carry = best.copy()
            sc = H._normalise((best + e[:, t]).astype(F))
    return H._walk_back(sc, bp), bp, sc, carry


def windows(logits, s, T, h, n):
    """n windows of T frames advancing by h over logits [512, >= (n - 1) h + T], each carried from the one before (the first from nothing)
    -> [(path, bp, sc, carry)]"""
    out, prior = [], None
    for k in range(n):
        out.append(viterbi_carried(logits[:, k * h:k * h + T], s, prior, h))
        prior = out[-1][3]
    return out


def planted_octave(margin):
    """ridge(20, 200, seed=1) with class 248 (an octave up) raised `margin` above class 200 from frame 8 on"""
    x = H.ridge(20, 200, seed=1)
    x[248, 8:] = x[200, 8:] + F(margin)
    return x
