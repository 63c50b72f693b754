"""The weighted match of include/tinyvc_hip.h ("weighted neighbours") restated in numpy fp32, operation by operation: every sum, product and
quotient below is ONE fp32 rounding, in the header's order, so a kernel that follows the definition agrees bit for bit."""
import numpy as np

F = np.float32


def weights(sims, k, width):
    """sims [..., 4] fp32 (s_0 >= ... >= s_3 as the lists hold them), k and width broadcastable to sims[..., 0] -> (w [..., 4], W [...])"""
    s = np.asarray(sims, F)
    k = np.clip(np.broadcast_to(np.asarray(k, np.int64), s.shape[:-1]), 1, 4)
    width = np.broadcast_to(np.asarray(width, F), s.shape[:-1])
    w = np.zeros(s.shape, F)
    w[..., 0] = 1
    with np.errstate(all="ignore"):
        for e in range(1, 4):
            g = (s[..., 0] - s[..., e]).astype(F)
            t = (g / width).astype(F)
            we = np.where(t > 0, np.maximum(F(0), (F(1) - t).astype(F)), F(1)).astype(F)      # NaN > 0 is False: 1
            w[..., e] = np.where(e < k, we, F(0))
    W = (((w[..., 0] + w[..., 1]).astype(F) + w[..., 2]).astype(F) + w[..., 3]).astype(F)
    return w, W


def weighted_mean(rows4, w, W):
    """rows4 [..., 4, C] fp32 (r_0 .. r_3 of every column), w [..., 4], W [...] -> mu [..., C]"""
    r = np.asarray(rows4, F)
    with np.errstate(all="ignore"):
        acc = r[..., 0, :].copy()
        for e in range(1, 4):
            we = w[..., e][..., None]
            term = (acc + (we * r[..., e, :]).astype(F)).astype(F)
            acc = np.where(we != 0, term, acc)      # a neighbour of weight 0 takes no part, whatever it holds
        return (acc / W[..., None]).astype(F)


def match(sims, idx, rows, k=4, width=np.inf):
    """The definition: sims [..., 4] fp32, idx [..., 4] ints into rows [N, C] fp32; k / width scalars or arrays broadcastable to sims[..., 0]
    -> mu [..., C] fp32"""
    w, W = weights(sims, k, width)
    return weighted_mean(np.asarray(rows, F)[np.asarray(idx)], w, W)


def mean4(rows4):
    """(((r0 + r1) + r2) + r3) * 0.25: the unweighted kernels' mean, rows4 [..., 4, C]"""
    r = np.asarray(rows4, F)
    return ((((r[..., 0, :] + r[..., 1, :]).astype(F) + r[..., 2, :]).astype(F) + r[..., 3, :]).astype(F) * F(0.25)).astype(F)


def planted_index(n=300, dim=768, seed=7):
    """(rows [n, dim], query [dim], a): unit row `a`, the query = that row plus small noise, three rows near 0.3 cosine to it, every other row
    close to orthogonal - the index on which a flat mean of four visibly blurs a row the index holds"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim)).astype(F)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    a = 17
    A = rows[a].copy()
    for j in (40, 41, 42):
        v = rows[j] - (rows[j] @ A) * A
        v /= np.linalg.norm(v)
        rows[j] = (F(0.3) * A + F(np.sqrt(1 - 0.09)) * v).astype(F)
    q = (A + F(0.01) * rng.standard_normal(dim).astype(F)).astype(F)
    return rows, q, a
