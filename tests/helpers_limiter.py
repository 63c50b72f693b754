"""The look-ahead peak limiter of include/tinyvc_hip.h restated in numpy fp32, operation by operation: every arithmetic step below is one
correctly rounded fp32 operation (numpy float32 scalars and arrays round each operation on its own), max / min / compare are exact, so
the kernels are held to these results bit for bit - gains and samples."""
import math

import numpy as np

F = np.float32


def ceiling_of(c):
    """the ceiling as the kernel reads it: NaN, <= 0 and +inf are off (+inf)"""
    c = F(c)
    return c if c > 0 else F(np.inf)


def drive_of(drive_db):
    """(float)10^(drive_db / 20): drive_db travels as fp32, the power is taken in double and rounded once"""
    return F(math.pow(10.0, float(F(drive_db)) / 20.0))


def peaks(v, sub):
    """p[k] = max |v| over sub-frame k, NaN samples ignored"""
    a = np.abs(v.reshape(-1, sub))
    return np.where(np.isnan(a), F(0), a).max(axis=1).astype(F) if a.size else np.zeros(0, F)


def ratios(p, c):
    """r[k], k = 0 .. K, from the peaks p[0 .. K - 1] with p[-1] = p[K] = 0"""
    pp = np.concatenate([[F(0)], p, [F(0)]]).astype(F)
    m = np.maximum(pp[:-1], pp[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m > c, (c / m).astype(F), F(1)).astype(F)


def step(e, r, d):
    return min(r, min(F(1), F(e + d)))


def recurrence(r, release, e=F(1), start=0):
    """e[k] = min(r[k], min(1, e[k-1] + d)) from e[start - 1] = e; entries before `start` are NaN"""
    d = F(F(1) / F(release))
    out = np.full(len(r), np.nan, F)
    for k in range(start, len(r)):
        e = step(e, r[k], d)
        out[k] = e
    return out


def ramp(v, e0, e1, sub, c):
    """sub-frames v [K, sub] between the edge gains e0 [K] and e1 [K]: the gate's ramp, then the clamp (NaN passes)"""
    t = (np.arange(1, sub + 1, dtype=F) / F(sub)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (e0[:, None] + ((e1 - e0).astype(F)[:, None] * t[None, :]).astype(F)).astype(F)
        o = (v * g).astype(F)
    return np.where(o > c, c, np.where(o < -c, -c, o)).astype(F)


def limit(y, ceiling, sub=24, release=100, drive_db=0.0, length=None):
    """one row, offline: (out, gains [L / sub + 1]); `length`: the row's own samples (clamped to 0 .. L, whole sub-frames of them); the
    samples behind them are copied and the gains behind its last edge are 1"""
    y = np.asarray(y, F)
    L = len(y)
    n = (L if length is None else max(0, min(int(length), L))) // sub
    c, drive = ceiling_of(ceiling), drive_of(drive_db)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (y[:n * sub] * drive).astype(F)
    e = recurrence(ratios(peaks(v, sub), c), release)
    out = y.copy()
    out[:n * sub] = ramp(v.reshape(n, sub), e[:-1], e[1:], sub, c).reshape(-1)
    gains = np.ones(L // sub + 1, F)
    gains[:n + 1] = e
    return out, gains


class Stream:
    """one stream: the state the kernel keeps (tail, peak, gain) and a block at a time"""

    def __init__(self, sub=24, release=100, drive_db=0.0):
        self.sub, self.release, self.drive = sub, release, drive_of(drive_db)
        self.tail, self.peak, self.gain = np.zeros(sub, F), F(0), F(1)

    def block(self, y, ceiling):
        """-> (out, gains [block / sub + 1]): the block delayed by one sub-frame"""
        y = np.asarray(y, F)
        sub, c = self.sub, ceiling_of(ceiling)
        with np.errstate(invalid="ignore", over="ignore"):
            v = (y * self.drive).astype(F)
        p = np.concatenate([[self.peak], peaks(v, sub)]).astype(F)
        m = np.maximum(p[:-1], p[1:])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(m > c, (c / m).astype(F), F(1)).astype(F)
        e = np.concatenate([[self.gain], recurrence(r, self.release, self.gain)]).astype(F)
        src = np.concatenate([self.tail, v[:-sub]]).reshape(-1, sub)
        out = ramp(src, e[:-1], e[1:], sub, c).reshape(-1)
        self.tail, self.peak, self.gain = v[-sub:].copy(), p[-1], e[-1]
        return out, e


def bursty(rng, n, sub, level=0.3, burst=4.0, bursts=()):
    """noise at `level` with `burst`-high sub-frames at the listed sub-frame indices"""
    y = (rng.standard_normal(n) * level).astype(F)
    for k in bursts:
        if 0 <= k < n // sub:
            y[k * sub:(k + 1) * sub] = (rng.choice([-1.0, 1.0], sub) * burst * rng.uniform(0.5, 1.0, sub)).astype(F)
            y[k * sub + sub // 2] = F(burst)
    return y


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)) or np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
