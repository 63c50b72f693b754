"""The loudness envelope match of include/tinyvc_hip.h, restated in fp64 on the host (numpy): the sub-frame powers, the gain from two window
sums, the offline gain sequence, a stream that carries its own rings, and the fp32 ramp with every operation rounded on its own.  Nothing
here touches the library."""
import math

import numpy as np

DEFAULTS = dict(sub=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0)


def constants(floor_db=-60.0, boost_db=12.0, cut_db=40.0):
    """(floor, lo, hi) in fp64 from the three settings as the C entry takes them (fp32 values)"""
    f, b, c = (float(np.float32(v)) for v in (floor_db, boost_db, cut_db))
    return 10.0 ** (f / 10.0), 10.0 ** (-c / 20.0), 10.0 ** (b / 20.0)


def share_value(e):
    """the share as the kernel reads it: an fp32 value clamped to [0, 1], NaN is 0"""
    e = float(np.float32(e))
    return 0.0 if math.isnan(e) else min(max(e, 0.0), 1.0)


def powers(v, sub):
    """v [n] fp32, n a multiple of sub -> the mean power of every sub-frame, squared and summed in fp64"""
    v = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1, sub)
    with np.errstate(invalid="ignore", over="ignore"):
        return (v * v).sum(axis=1) / float(sub)


def gain(sum_s, sum_o, cnt, e, consts):
    """the gain of a sub-frame from the sums of its two windows of cnt powers, rounded to fp32 once"""
    floor, lo, hi = consts
    if e == 0.0 or not math.isfinite(sum_s) or not math.isfinite(sum_o):
        return np.float32(1.0)
    q = max(sum_s / cnt, floor) / max(sum_o / cnt, floor)
    r = float(np.exp2(0.5 * e * np.log2(q)))
    return np.float32(min(max(r, lo), hi))


def _ascending(p, lo, hi):
    s = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(lo, hi + 1):
            s = s + float(p[k])
    return s


def offline_edges(x, y, e, length=None, sub=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0):
    """one row of tvc_loudness_match_f32: x, y [L] fp32, the row's own length (None: L) -> the gain at every sub-frame edge, fp32 [L / sub + 1]:
    edge 0 and edge 1 the first sub-frame's gain, edge i + 1 sub-frame i's, 1 behind the row's length"""
    L = len(y)
    n = (L if length is None else min(max(int(length), 0), L)) // sub
    ps, po = powers(x[:n * sub], sub), powers(y[:n * sub], sub)
    consts, e = constants(floor_db, boost_db, cut_db), share_value(e)
    edges = np.ones(L // sub + 1, dtype=np.float32)
    for i in range(n):
        lo, hi = max(i - smooth, 0), min(i + smooth, n - 1)
        edges[i + 1] = gain(_ascending(ps, lo, hi), _ascending(po, lo, hi), hi - lo + 1, e, consts)
    if n:
        edges[0] = edges[1]
    return edges


class StreamRestatement:
    """one stream of tvc_stream_loudness_f32 with its own state: rings [W] fp64 (slot = sub-frame index % W), frames, gain"""

    def __init__(self, sub=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0):
        self.sub, self.W = sub, 2 * smooth + 1
        self.consts = constants(floor_db, boost_db, cut_db)
        self.src_ring, self.out_ring = np.zeros(self.W), np.zeros(self.W)
        self.frames, self.gain = 0, np.float32(1.0)

    def block(self, window, y, start, e):
        """window [n] fp32 the stream's input window, y [block] the emitted block, start = base + shift -> the block's edge gains
        [block / sub + 1] (edge 0: the carried gain, or the first sub-frame's own at the start of the stream)"""
        window, y = np.asarray(window, dtype=np.float32), np.asarray(y, dtype=np.float32)
        idx = start + np.arange(len(y))
        ok = (idx >= 0) & (idx < len(window))
        src = np.where(ok, window[np.clip(idx, 0, len(window) - 1)], np.float32(0.0)).astype(np.float32)
        ps, po = powers(src, self.sub), powers(y, self.sub)
        e = share_value(e)
        edges = np.empty(len(ps) + 1, dtype=np.float32)
        edges[0] = self.gain
        for i in range(len(ps)):
            self.src_ring[self.frames % self.W], self.out_ring[self.frames % self.W] = ps[i], po[i]
            cnt = min(self.frames + 1, self.W)
            order = [(self.frames - cnt + 1 + k) % self.W for k in range(cnt)]      # oldest to newest
            edges[i + 1] = gain(_ascending(self.src_ring[order], 0, cnt - 1), _ascending(self.out_ring[order], 0, cnt - 1), cnt, e, self.consts)
            if self.frames == 0:
                edges[0] = edges[1]
            self.frames += 1
        self.gain = edges[-1]
        return edges


def ramp(y, edges, sub):
    """y [n] fp32 under the edge gains [n / sub + 1]: sample j of sub-frame i times g0 + (g1 - g0) * ((j + 1) / sub), each operation an fp32
    operation of its own"""
    y = np.asarray(y, dtype=np.float32).reshape(-1, sub)
    edges = np.asarray(edges, dtype=np.float32)
    g0, g1 = edges[:-1, None], edges[1:, None]
    t = np.arange(1, sub + 1, dtype=np.float32)[None, :] / np.float32(sub)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (g1 - g0).astype(np.float32)
        m = (g0 + (d * t).astype(np.float32)).astype(np.float32)
        return (y * m).astype(np.float32).reshape(-1)


def ulps(a, b):
    """the largest distance in fp32 steps between two arrays of positive finite fp32 numbers"""
    a, b = (np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return int(np.abs(a - b).max()) if a.size else 0
