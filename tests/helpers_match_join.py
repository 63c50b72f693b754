"""The match along a path of include/tinyvc_hip.h ("match along a path") restated in numpy fp32, operation by operation, on the pieces of
helpers_match_weight.py: every sum, product and quotient below is ONE fp32 rounding, in the header's order, so a kernel that follows the
definition agrees bit for bit."""
import numpy as np

from helpers_match_weight import F

BIG = np.finfo(np.float32).max


def sat(x):
    """fminf(fmaxf(x, -FLT_MAX), FLT_MAX); NaN -> -FLT_MAX"""
    x = np.asarray(x, F)
    return np.where(np.isnan(x), F(-BIG), np.clip(x, F(-BIG), F(BIG))).astype(F)


def finite(x):
    """a similarity or an affinity that is not finite counts as 0"""
    x = np.asarray(x, F)
    return np.where(np.isfinite(x), x, F(0)).astype(F)


def continuity(c):
    """NaN and negatives count as 0, +inf as the largest finite float"""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.minimum(c, F(BIG)), F(0)).astype(F)


def dot(u, v):
    """the one order of the header: u, v [..., 768] fp32 -> [...]: 64 partial sums over channels l, l + 64, .., l + 704 (ascending), then the
    butterfly over distances 32, 16, 8, 4, 2, 1"""
    p = (np.asarray(u, F) * np.asarray(v, F)).astype(F)
    p = p.reshape(p.shape[:-1] + (12, 64))
    P = p[..., 0, :]
    for j in range(1, 12):
        P = (P + p[..., j, :]).astype(F)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        P = (P + P[..., lanes ^ m]).astype(F)
    return P[..., 0]


def affinities(rows, inv, idx):
    """rows [N, 768] fp32 as the blob holds them, inv [N] fp32 = 1 / (|v| + 1e-6) as the blob holds it, idx [len, 4] -> a [len, 4, 4] fp32
    ([t][d][e] against frame t - 1; frame 0: zeros)"""
    rows, inv, idx = np.asarray(rows, F), np.asarray(inv, F), np.asarray(idx)
    a = np.zeros((idx.shape[0], 4, 4), F)
    if idx.shape[0] > 1:
        prev, cur = idx[:-1], idx[1:]
        d = dot(rows[prev][:, :, None, :], rows[cur][:, None, :, :])
        a[1:] = ((d * inv[prev][:, :, None]).astype(F) * inv[cur][:, None, :]).astype(F)
    return a


def blob_inv(rows):
    """inv = 1 / (|v| + 1e-6) in fp64, rounded once: what a reference may use where the blob's own is not at hand"""
    r = np.asarray(rows, np.float64)
    return (1.0 / (np.sqrt((r * r).sum(-1)) + 1e-6)).astype(F)


def paths(sims, aff, k=4, c=0.0, want_scores=False):
    """U utterances of one length: sims [U, len, 4] fp32, aff [U, len, 4, 4] fp32 (frame 0 ignored), k ints and c floats broadcastable to
    [U] -> anchors [U, len] int32 (, the last frame's renormalised scores [U, 4]).  States from k on take no part: masked out of every
    maximum, their scores are whatever the recursion leaves."""
    s = finite(sims)
    a = finite(aff)
    U, n = s.shape[:2]
    k = np.clip(np.broadcast_to(np.asarray(k, np.int64), (U,)), 1, 4)
    c = continuity(np.broadcast_to(np.asarray(c, F), (U,)))
    live = np.arange(4)[None, :] < k[:, None]                        # [U, state]
    bp = np.zeros((U, n, 4), np.int32)
    D = np.zeros((U, 4), F)
    with np.errstate(all="ignore"):
        for t in range(n):
            if t == 0:
                x = s[:, 0].copy()
            else:
                jc = sat((c[:, None, None] * a[:, t]).astype(F))     # [U][d][e]
                cand = (D[:, :, None] + jc).astype(F)
                best = cand[:, 0].copy()
                for d in range(1, 4):
                    take = live[:, d, None] & (cand[:, d] > best)    # ties keep the lowest d
                    best = np.where(take, cand[:, d], best)
                    bp[:, t] = np.where(take, d, bp[:, t])
                x = sat((s[:, t] + best).astype(F))
            mx = np.where(live, x, F(-np.inf)).max(axis=1)
            D = sat((x - mx[:, None]).astype(F))
    p = np.zeros(U, np.int64)
    best = D[:, 0].copy()
    for e in range(1, 4):
        take = live[:, e] & (D[:, e] > best)
        best = np.where(take, D[:, e], best)
        p = np.where(take, e, p)
    anchors = np.zeros((U, n), np.int32)
    rows = np.arange(U)
    for t in range(n - 1, -1, -1):
        anchors[:, t] = p
        p = bp[rows, t, p]
    return (anchors, D) if want_scores else anchors


def path(sims, aff, k=4, c=0.0, want_scores=False):
    """ONE utterance: sims [len, 4], aff [len, 4, 4], k an int, c a float -> anchors [len] int32 (, the last frame's scores [4])"""
    res = paths(np.asarray(sims, F)[None], np.asarray(aff, F)[None], k, c, want_scores)
    return (res[0][0], res[1][0]) if want_scores else res[0]


def weights(sims, anchor, k, width):
    """helpers_match_weight.weights around an anchor: sims [..., 4] fp32 (RAW, as sims_out holds them), anchor [...] ints, k and width
    broadcastable to sims[..., 0] -> (w [..., 4], W [...])"""
    s = np.asarray(sims, F)
    p = np.asarray(anchor, np.int64) & 3
    k = np.clip(np.broadcast_to(np.asarray(k, np.int64), s.shape[:-1]), 1, 4)
    width = np.broadcast_to(np.asarray(width, F), s.shape[:-1])
    sp = np.take_along_axis(s, p[..., None], -1)[..., 0]
    w = np.zeros(s.shape, F)
    with np.errstate(all="ignore"):
        for e in range(4):
            g = np.abs((sp - s[..., e]).astype(F))
            t = (g / width).astype(F)
            we = np.where(t > 0, np.maximum(F(0), (F(1) - t).astype(F)), F(1)).astype(F)
            w[..., e] = np.where(p == e, F(1), np.where(e < k, we, F(0)))
    W = (((w[..., 0] + w[..., 1]).astype(F) + w[..., 2]).astype(F) + w[..., 3]).astype(F)
    return w, W


def anchored_mean(rows4, w, W):
    """rows4 [..., 4, C] fp32, w [..., 4], W [...] -> mu [..., C]: the terms of weight != 0 in ascending e, the first starting the sum"""
    r = np.asarray(rows4, F)
    acc = np.zeros(r.shape[:-2] + r.shape[-1:], F)
    started = np.zeros(r.shape[:-2] + (1,), bool)
    with np.errstate(all="ignore"):
        for e in range(4):
            we = w[..., e][..., None]
            term = (we * r[..., e, :]).astype(F)
            acc = np.where(we != 0, np.where(started, (acc + term).astype(F), term), acc)
            started = started | (we != 0)
        return (acc / W[..., None]).astype(F)


def match(sims, idx, rows, anchor, k=4, width=np.inf):
    """The definition behind the path: sims [..., 4], idx [..., 4] ints into rows [N, C], anchor [...] -> mu [..., C] fp32"""
    w, W = weights(sims, anchor, k, width)
    return anchored_mean(np.asarray(rows, F)[np.asarray(idx)], w, W)


def flips(rows_of_anchor, in_a):
    """how often the anchor's row changes set between neighbouring frames: rows_of_anchor [len] ints, in_a a set of the chain's rows"""
    side = np.array([int(r) in in_a for r in rows_of_anchor])
    return int((side[1:] != side[:-1]).sum())


def planted_chain(n=300, dim=768, frames=12, seed=11, gain=0.004):
    """(rows [n, dim], queries [frames, dim], chain [frames], strangers [frames], margin): on top of an index of near-orthogonal unit rows,
    a chain A of rows that are mutually close from frame to frame (cosine about 0.9 between neighbours) and a set B of rows far from A and from
    each other.  Query t lies between A[t] and B[t], nearer by `gain` in cosine to B on even frames and to A on odd ones: frame by frame
    the nearest row alternates between the sets, along a path it stays in A once the continuity weight outweighs the margin.
    margin = the largest similarity lead B ever has over A, an upper bound from the construction (2 * gain covers fp32 rounding)."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim)).astype(np.float64)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    chain = np.arange(20, 20 + frames)
    strangers = np.arange(100, 100 + frames)
    base = rows[5].copy()
    for t, r in enumerate(chain):      # A[t] = the base direction plus a small part of its own: neighbours 0.9 alike
        own = rows[r] - (rows[r] @ base) * base
        own /= np.linalg.norm(own)
        rows[r] = np.sqrt(0.9) * base + np.sqrt(0.1) * own
    queries = np.zeros((frames, dim))
    for t in range(frames):
        A, B = rows[chain[t]], rows[strangers[t]]
        lead = gain if t % 2 == 0 else -gain      # B's lead over A
        # q = cos(phi) A' + sin(phi) B' in the plane of A and B; the lead moves with the angle from the bisector
        b = B - (B @ A) * A
        b /= np.linalg.norm(b)
        ang = np.arccos(np.clip(A @ B, -1, 1))
        phi = ang / 2 + lead / (2 * np.sin(ang / 2))      # d(cos(phi - ang) - cos(phi)) / d phi at the bisector = 2 sin(ang / 2)
        queries[t] = np.cos(phi) * A + np.sin(phi) * b
    return rows.astype(F), queries.astype(F), chain, strangers, 2 * gain
