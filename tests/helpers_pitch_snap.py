"""The pitch correction of include/tinyvc_hip.h (tvc_pitch_snap_f32) restated in numpy fp32, operation by operation: every product, sum,
difference and quotient is one rounded fp32 operation, sqrt is numpy's correctly rounded one, compares, min and max are exact.  No
transcendentals, so the kernel is held to this bit for bit.  Also the host's table builder (a second statement of
feature_retrieval.note_table), the sanitising rules for the table, the strength and a carried state, and the carry itself."""
import numpy as np

F = np.float32
NOTES = 128
RATIO_MIN = np.array([0x3F2AAAAB], dtype=np.uint32).view(F)[0]      # 2/3f
RATIO_MAX = F(1.5)
SCALES = {"chromatic": range(12), "major": (0, 2, 4, 5, 7, 9, 11), "minor": (0, 2, 3, 5, 7, 8, 10), "pentatonic": (0, 2, 4, 7, 9)}
KEYS = {"C": 0, "C#": 1, "Db": 1, "D": 2, "D#": 3, "Eb": 3, "E": 4, "F": 5, "F#": 6, "Gb": 6, "G": 7, "G#": 8, "Ab": 8, "A": 9, "A#": 10, "Bb": 10, "B": 11}


def midi_hz(m, a4=440.0):
    """a4 * 2^((m - 69) / 12) in fp64, rounded to fp32 once"""
    return F(float(a4) * 2.0 ** ((float(m) - 69.0) / 12.0))


def note_table(key="C", scale="major", notes=None, a4=440.0, low=24, high=96):
    """-> (fp32 [128] ascending, padded with +inf; the number of notes)"""
    if notes is None:
        degrees = {(KEYS[key] + d) % 12 for d in SCALES[scale]}
        notes = [m for m in range(low, high + 1) if m % 12 in degrees]
    notes = sorted(set(notes))
    assert 1 <= len(notes) <= NOTES
    table = np.full(NOTES, np.inf, dtype=F)
    table[:len(notes)] = [midi_hz(m, a4) for m in notes]
    return table, len(notes)


def settings(table, n, retune_ms=60.0, hysteresis_cents=25.0):
    """PitchSnap's host values from its arguments: (h, g, f_min, f_max) as fp32"""
    g = 1.0 if retune_ms == 0 else 1.0 - np.exp(-20.0 / retune_ms)
    h = 2.0 ** (hysteresis_cents / 1200.0)
    semi = 2.0 ** (1.0 / 12.0)
    return F(h), F(g), F(max(float(table[0]) / semi, 32.0)), F(float(table[n - 1]) * semi)


def table_size(notes):
    """K: the largest k with notes[0 .. k-1] finite, notes[0] > 0 and strictly ascending"""
    notes = np.asarray(notes, dtype=F)
    K, before = 0, F(0)
    for v in notes[:NOTES]:
        if not (np.isfinite(v) and v > before):
            break
        K, before = K + 1, v
    return K


def bounds(notes, h):
    """-> (K, b [K-1], lo [K], hi [K])"""
    notes, h = np.asarray(notes, dtype=F), F(h)
    K = table_size(notes)
    with np.errstate(over="ignore"):
        b = np.sqrt(notes[:max(K - 1, 0)] * notes[1:max(K, 1)]).astype(F)
        lo = np.zeros(K, dtype=F)
        hi = np.full(K, np.inf, dtype=F)
        if K > 1:
            lo[1:] = b / h
            hi[:-1] = b * h
    assert b.dtype == lo.dtype == hi.dtype == F
    return K, b, lo, hi


def clean_strength(s):
    s = F(s)
    return F(0) if np.isnan(s) else min(max(s, F(0)), F(1))


def clean_prior(prior, K):
    """a state as the kernel takes it, whatever was written there: (q, c)"""
    if prior is None:
        return -1, F(1)
    note, ratio = int(prior[0]), F(prior[1])
    if 0 <= note < K and RATIO_MIN <= ratio <= RATIO_MAX:      # a NaN fails the compare
        return note, ratio
    return -1, F(1)


def snap_row(x, notes, h, g, f_min, f_max, strength=1.0, prior=None, carry_frame=0):
    """one row -> (out fp32 [T], note_out int32 [T], state (note, ratio) behind frame carry_frame - 1 or None)"""
    x = np.asarray(x, dtype=F)
    notes = np.asarray(notes, dtype=F)
    g, f_min, f_max = F(g), F(f_min), F(f_max)
    K, b, lo, hi = bounds(notes, h)
    s = clean_strength(strength)
    q, c = clean_prior(prior, K)
    out, note_out, state = x.copy(), np.full(len(x), -1, dtype=np.int32), None
    one = F(1)
    for t in range(len(x)):
        v = x[t]
        if not (K > 0 and f_min <= v and v <= f_max):
            q = -1
        else:
            n = q if q >= 0 and lo[q] < v and v < hi[q] else int(np.sum(b <= v))
            r = notes[n] / v
            c = r if q < 0 else c + g * (r - c)
            c = min(max(c, RATIO_MIN), RATIO_MAX)
            q = n
            out[t] = v * (one + s * (c - one))
            note_out[t] = n
            assert type(c) is F and out.dtype == F
        if t == carry_frame - 1:
            state = (q, c if q >= 0 else F(1))
    return out, note_out, state


def snap_rows(f0, row_start, row_count, notes, h, g, f_min, f_max, strength=None, state=None, carry_frame=0):
    """the stage call over a flat f0: -> (out like f0, note_out int32 like f0, new state (note int32 [rows], ratio fp32 [rows]) or None).
    Columns outside every row are not written: they keep f0's value in out and hold -7 in note_out.  An empty row keeps its state."""
    f0 = np.asarray(f0, dtype=F)
    out, note_out = f0.copy(), np.full(f0.shape, -7, dtype=np.int32)
    new = None if state is None else (np.array(state[0], dtype=np.int32), np.array(state[1], dtype=F))
    for i, (a, n) in enumerate(zip(row_start, row_count)):
        if n <= 0:
            continue
        o, k, st = snap_row(f0[a:a + n], notes, h, g, f_min, f_max, 1.0 if strength is None else strength[i],
                            None if state is None else (state[0][i], state[1][i]), carry_frame if state is not None else 0)
        out[a:a + n], note_out[a:a + n] = o, k
        if new is not None:
            new[0][i], new[1][i] = st
    return out, note_out, new


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, dtype=np.float64) / float(ref))
