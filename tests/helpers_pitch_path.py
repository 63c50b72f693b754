"""The pitch path of include/tinyvc_hip.h restated in numpy fp32, operation by operation: every arithmetic step below is one correctly
rounded fp32 operation (numpy float32 arrays round each operation on its own), max / compare / argmax are exact and np.argmax returns the
FIRST maximum, so the kernel is held to these results bit for bit - classes, back-pointers and scores.

Two forms.  `viterbi_full` is the definition: all 512 x 512 candidates of a frame.  `viterbi_banded` is what the kernel computes: the band's
2 W + 1 candidates per class, the class-0 candidate, and ONE reduction per frame for the far ones - the maximum and its lowest class of
s[i] - jump over ALL voiced classes.  That is the same thing because jump >= W * step and rounding is monotone: for a class i inside the band
of j, s[i] - jump <= s[i] - |i - j| * step, so the jump route never beats the band, and where the reduction's winner lies inside the band
the band holds a class at least as good and, on equal values, no higher.  tests/test_pitch_path_host.py holds the two equal bit for bit."""
import collections

import numpy as np

F = np.float32
CLASSES = 512
CLAMP = F(1e30)
Settings = collections.namedtuple("Settings", "step band jump voicing refine")
DEFAULT = Settings(0.5, 12, 12.0, 3.0, 2)      # guesses: nobody has listened


def emission(logits):
    """e = x clamped to [-1e30, 1e30], NaN -> -1e30; logits [512, T]"""
    x = np.asarray(logits, dtype=F)
    return np.where(np.isnan(x), -CLAMP, np.minimum(np.maximum(x, -CLAMP), CLAMP)).astype(F)


def cost_matrix(s):
    """cost[i, j] of the definition, fp32"""
    i, j = np.meshgrid(np.arange(CLASSES), np.arange(CLASSES), indexing="ij")
    d = np.abs(i - j)
    c = np.where(d <= s.band, d.astype(F) * F(s.step), F(s.jump)).astype(F)
    c[0, :] = c[:, 0] = F(s.voicing)
    c[0, 0] = F(0)
    return c


def _normalise(u):
    return (u - u.max()).astype(F)


def _walk_back(last, bp):
    T = bp.shape[0]
    path = np.zeros(T, np.int32)
    path[T - 1] = int(np.argmax(last))
    for t in range(T - 1, 0, -1):
        path[t - 1] = bp[t, path[t]]
    return path


def viterbi_full(logits, s):
    """the definition -> (path [T] int32, bp [T, 512] (row 0 unused), s_{T-1} [512] fp32)"""
    e = emission(logits)
    T = e.shape[1]
    cost = cost_matrix(s)
    bp = np.zeros((T, CLASSES), np.int32)
    sc = _normalise(e[:, 0])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            cand = (sc[:, None] - cost).astype(F)      # cand[i, j]
            bp[t] = np.argmax(cand, axis=0)            # the lowest i on equal values
            sc = _normalise((cand.max(axis=0) + e[:, t]).astype(F))
    return _walk_back(sc, bp), bp, sc


def viterbi_banded(logits, s):
    """the kernel's shortcut, same outputs"""
    e = emission(logits)
    T = e.shape[1]
    W, step, jump, voicing = int(s.band), F(s.step), F(s.jump), F(s.voicing)
    bp = np.zeros((T, CLASSES), np.int32)
    sc = _normalise(e[:, 0])
    js = np.arange(1, CLASSES)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            best, frm = np.empty(CLASSES, F), np.zeros(CLASSES, np.int32)
            # class 0: from itself for nothing, or from the best voiced class at `voicing`
            vv = (sc[1:] - voicing).astype(F)
            best[0] = sc[0]
            if vv.max() > best[0]:
                best[0], frm[0] = vv.max(), 1 + int(np.argmax(vv))
            # voiced classes: from class 0, then the band in ascending order (`>` keeps the lowest), then the one far candidate
            b = np.full(CLASSES - 1, sc[0] - voicing, F)
            f = np.zeros(CLASSES - 1, np.int32)
            pad = np.full(CLASSES + 2 * W, -np.inf, F)
            pad[W + 1:W + CLASSES] = sc[1:]            # class 0's slot and the pads hold -inf
            for d in range(-W, W + 1):
                cand = (pad[W + js + d] - F(abs(d)) * step).astype(F)
                take = cand > b
                b, f = np.where(take, cand, b), np.where(take, js + d, f)
            vj = (sc[1:] - jump).astype(F)
            fv, fi = vj.max(), 1 + int(np.argmax(vj))
            take = (fv > b) | ((fv == b) & (fi < f))
            best[1:], frm[1:] = np.where(take, fv, b), np.where(take, fi, f)
            bp[t] = frm
            sc = _normalise((best + e[:, t]).astype(F))
    return _walk_back(sc, bp), bp, sc


def frequency(logits, path, refine, freq):
    """f0 [T] fp32 of a path, the kernel's arithmetic: quotient, product and sum rounded separately, exp in fp64 rounded once"""
    e, freq = emission(logits), np.asarray(freq, dtype=F)
    out = np.zeros(len(path), F)
    for t, c in enumerate(path):
        if c == 0:
            continue
        lo, hi = max(1, c - refine), min(CLASSES - 1, c + refine)
        x = e[lo:hi + 1, t]
        w = np.exp((x - x.max()).astype(F).astype(np.float64)).astype(F)
        den = w[0]
        for v in w[1:]:
            den = F(den + v)
        acc = None
        for v, fr in zip(w, freq[lo:hi + 1]):
            term = F(F(v / den) * fr)
            acc = term if acc is None else F(acc + term)
        out[t] = acc if acc > F(20) else F(0)
    return out


def frequency64(logits, path, refine, freq):
    """the same expectation in fp64 on the fp32 emissions, without the gate -> [T] float64"""
    e, freq = emission(logits).astype(np.float64), np.asarray(freq, dtype=np.float64)
    out = np.zeros(len(path))
    for t, c in enumerate(path):
        if c == 0:
            continue
        lo, hi = max(1, c - refine), min(CLASSES - 1, c + refine)
        w = np.exp(e[lo:hi + 1, t] - e[lo:hi + 1, t].max())
        out[t] = (w * freq[lo:hi + 1]).sum() / w.sum()
    return out


def f0_bound(refine):
    """relative to the fp64 value: four roundings for each of the 2 r + 1 terms plus the 2 r adds of the denominator, half an ulp = 2^-24
    each, first order (derived as item 3 of test_gpu_front_dsp_edges.py's docstring derives its 16)"""
    return (4 * (2 * refine + 1) + 2 * refine) * 2.0 ** -24


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def gaussian(T, seed):
    return np.random.default_rng(seed).standard_normal((CLASSES, T)).astype(F)


def quantised(T, seed, levels=9):
    """multiples of 0.25 in a narrow range: every sum and difference is exact and equal values are everywhere"""
    return (np.random.default_rng(seed).integers(0, levels, (CLASSES, T)) * 0.25).astype(F)


def ridge(T, c, height=8.0, seed=0, noise=0.25):
    """a ridge at class c over a low noisy floor"""
    x = (-4.0 + noise * np.random.default_rng(seed).standard_normal((CLASSES, T))).astype(F)
    x[c] = F(height)
    return x


def planted_flip(T, c, t, margin, seed=0):
    """a ridge at class c whose frame t has class c + 48 (an octave up) higher by `margin`"""
    x = ridge(T, c, seed=seed)
    x[c + 48, t] = x[c, t] + F(margin)
    return x


def planted_dropout(T, c, t, margin, seed=0):
    """a ridge at class c whose frame t has class 0 higher by `margin`"""
    x = ridge(T, c, seed=seed)
    x[0, t] = x[c, t] + F(margin)
    return x


def special_columns(T, seed):
    """Gaussian logits with NaN, +inf and -inf sprinkled in, one all-NaN column, one all -inf and one all +inf"""
    r = np.random.default_rng(seed)
    x = r.standard_normal((CLASSES, T)).astype(F)
    for v in (np.nan, np.inf, -np.inf):
        x[r.integers(0, CLASSES, 3 * T), r.integers(0, T, 3 * T)] = v
    if T >= 8:
        x[:, 2], x[:, 4], x[:, 6] = np.nan, -np.inf, np.inf
    return x
