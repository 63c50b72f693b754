"""Pitch correction without a GPU: the numpy restatement's own properties (tests/helpers_pitch_snap.py), what the correction is for - vibrato
passes while the note's centre moves, a pitch on the bound between two notes does not flutter -, and the host side: PitchSnap, SnapCarry,
the parsers, stream_state.SNAP_STATE and the C prototypes.  Nobody has listened to any of it."""
import argparse
import math
import os
import re

import numpy as np
import pytest
import torch

import helpers_pitch_snap as H
from tinyvc_amd import _lib, stream_state
from tinyvc_amd.module.tinyvc import feature_retrieval as FR
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchSnap, SnapCarry

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAJOR, N_MAJOR = H.note_table("C", "major")
A3 = H.midi_hz(57)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _random_f0(n, seed):
    r = np.random.default_rng(seed)
    x = np.exp(r.uniform(np.log(40.0), np.log(1500.0), n))
    walk = 220.0 * 2.0 ** (np.cumsum(r.normal(0, 15, n)) / 1200.0)
    x = np.where(r.random(n) < 0.5, walk, x).astype(F)
    x[r.random(n) < 0.15] = 0
    x[r.integers(0, n, 6)] = [np.nan, -50.0, np.inf, -np.inf, 31.0, 1e30]
    return x


# ---- the helper's own properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_windows_over_one_tensor_equal_the_run_over_the_prefix(seed):
    T, hop, nwin = 28, 4, 12
    s = H.settings(MAJOR, N_MAJOR)
    x = _random_f0((nwin - 1) * hop + T, seed)
    state = None
    for n in range(nwin):
        out, note, state = H.snap_row(x[n * hop:n * hop + T], MAJOR, *s, strength=0.7, prior=state, carry_frame=hop)
        p_out, p_note, _ = H.snap_row(x[:n * hop + T], MAJOR, *s, strength=0.7)
        assert np.array_equal(_bits(out), _bits(p_out[n * hop:])) and np.array_equal(note, p_note[n * hop:]), f"window {n}"
        assert state[0] == p_note[n * hop + hop - 1] and (state[0] >= 0 or state[1] == 1.0)


def test_identities():
    s = H.settings(MAJOR, N_MAJOR)
    x = _random_f0(400, 5)
    out, note, _ = H.snap_row(x, MAJOR, *s, strength=0.0)
    assert np.array_equal(_bits(out), _bits(x)) and (note >= 0).any(), "s = 0 must return the input bits"
    one = np.full(128, np.inf, F)
    one[0] = 300.0
    out, note, _ = H.snap_row(x, one, F(1.0), F(1.0), F(32.0), F(2000.0))
    inr = (x >= 32.0) & (x <= 2000.0)
    assert (note[inr] == 0).all() and (note[~inr] == -1).all()
    assert (np.abs(H.cents(out[inr], 300.0)) <= np.abs(H.cents(x[inr], 300.0)) + 1e-3).all(), "a frame moved away from the one note"
    assert np.array_equal(_bits(out[~inr]), _bits(x[~inr]))
    near = inr & (x > 200.0) & (x < 450.0)      # inside the clamp of [2/3, 1.5] the one note is reached
    assert np.abs(H.cents(out[near], 300.0)).max() < 1e-3
    # g = 1, h = 1: the memoryless nearest-note snap
    out, note, _ = H.snap_row(x, MAJOR, F(1.0), F(1.0), s[2], s[3])
    K, b, _lo, _hi = H.bounds(MAJOR, F(1.0))
    for t in np.nonzero(note >= 0)[0]:
        n = int(np.sum(b <= x[t]))
        assert note[t] == n and out[t] == x[t] * (F(1) + F(1) * (min(max(MAJOR[n] / x[t], H.RATIO_MIN), H.RATIO_MAX) - F(1)))


def test_garbage_priors_and_tables_are_sanitised():
    assert H.RATIO_MIN.view(np.uint32) == 0x3F2AAAAB
    for prior in ((1000, 1.0), (-5, 1.0), (3, np.nan), (3, 9.0), (N_MAJOR, 1.0), (3, 0.66), (2 ** 31 - 1, 1.0)):
        assert H.clean_prior(prior, N_MAJOR) == (-1, F(1)), prior
    assert H.clean_prior((N_MAJOR - 1, 1.5), N_MAJOR) == (N_MAJOR - 1, F(1.5)) and H.clean_prior((0, H.RATIO_MIN), N_MAJOR) == (0, H.RATIO_MIN)
    assert [float(H.clean_strength(s)) for s in (0.0, 1.0, 0.5, np.nan, 7.0, -1.0, np.inf)] == [0.0, 1.0, 0.5, 0.0, 1.0, 0.0, 1.0]
    t = MAJOR.copy()
    assert H.table_size(t) == 43
    for i, v, K in ((20, np.nan, 20), (20, t[19], 20), (20, t[18], 20), (0, 0.0, 0), (0, -3.0, 0), (5, np.inf, 5), (42, np.inf, 42)):
        u = t.copy()
        u[i] = v
        assert H.table_size(u) == K, (i, v)
    u = t.copy()
    u[20] = np.nan
    x = _random_f0(300, 8)
    out, note, _ = H.snap_row(x, u, *H.settings(MAJOR, N_MAJOR))
    assert note.max() == 19 and (note >= 0).any()
    out, note, _ = H.snap_row(x, np.full(128, np.inf, F), *H.settings(MAJOR, N_MAJOR))
    assert np.array_equal(_bits(out), _bits(x)) and (note == -1).all()


@pytest.mark.parametrize("seed", range(8))
def test_no_in_range_frame_falls_under_the_voicing_gate(seed):
    r = np.random.default_rng(seed)
    table = np.full(128, np.inf, F)
    K = int(r.integers(1, 129))
    table[:K] = np.sort(np.exp(r.uniform(np.log(1e-3), np.log(1e6), K)).astype(F))
    table[:K] = np.maximum.accumulate(table[:K])
    x = np.exp(r.uniform(np.log(20.0), np.log(5000.0), 500)).astype(F)
    f_min, f_max = F(32.0 + 50 * r.random()), F(200.0 + 4000 * r.random())
    out, note, _ = H.snap_row(x, table, F(1.0 + 0.059 * r.random()), F(max(r.random(), 1e-3)), f_min, f_max, strength=r.random() * 1.5)
    inr = (x >= f_min) & (x <= f_max)
    assert ((note >= 0) == (inr & (H.table_size(table) > 0))).all()
    assert (out[note >= 0] > 20).all() and np.array_equal(_bits(out[note < 0]), _bits(x[note < 0]))
    assert (out[note >= 0] >= F(32) * H.RATIO_MIN).all()


# ---- the point --------------------------------------------------------------------------------------------------------------------------------------
def _vibrato():
    t = np.arange(400) * 0.02
    return (220.0 * 2.0 ** ((-30.0 + 40.0 * np.sin(2 * np.pi * 6.0 * t)) / 1200.0)).astype(F)


def test_vibrato_passes_while_the_centre_moves():
    """a tone 30 cents flat of A3 with 6 Hz vibrato of +-40 cents: at g = 0.1 the mean lands on the note and the vibrato survives; at g = 1
    it is flattened"""
    h, _g, f_min, f_max = H.settings(MAJOR, N_MAJOR)
    x = _vibrato()
    assert abs(float(H.cents(x[50:], A3).mean()) + 30.0) < 1.0
    out, note, _ = H.snap_row(x, MAJOR, h, F(0.1), f_min, f_max)
    c = H.cents(out[50:], A3)
    print(f"g = 0.1: mean {c.mean():.2f} cents, peak to peak {c.max() - c.min():.1f} of 80")
    assert (note == 19).all() and abs(c.mean()) < 1.0 and c.max() - c.min() > 70.0
    out, _n, _ = H.snap_row(x, MAJOR, h, F(1.0), f_min, f_max)
    c = H.cents(out[50:], A3)
    # exactly the note up to the roundings of div, sub, add and mul: four half-ulps of 2^-24 to either side are 8 * 2^-24 * 1200 / ln 2 cents
    assert c.max() - c.min() < 8 * 2.0 ** -24 * 1200 / math.log(2.0) and abs(c.mean()) < 1e-3


def test_hysteresis_stops_the_flutter():
    """a pitch on the bound between A3 and B3 under Gaussian noise of 8 cents: 206 changes of note without hysteresis, one at 25 cents"""
    bound = math.sqrt(float(H.midi_hz(57)) * float(H.midi_hz(59)))
    x = (bound * 2.0 ** (np.random.default_rng(0).normal(0, 8, 400) / 1200.0)).astype(F)
    changes = []
    for cents in (0.0, 25.0):
        out, note, _ = H.snap_row(x, MAJOR, *H.settings(MAJOR, N_MAJOR, hysteresis_cents=cents))
        assert set(note) <= {19, 20}
        changes.append(int(np.sum(note[1:] != note[:-1])))
    print(f"changes of note: {changes[0]} at 0 cents of hysteresis, {changes[1]} at 25")
    assert changes[0] > 100 and changes[1] <= 2


# ---- PitchSnap, SnapCarry, the parsers -----------------------------------------------------------------------------------------------------------------
def test_the_table_and_the_host_values():
    s = PitchSnap()
    assert s.n_notes == 43 and tuple(s.notes.shape) == (128,) and s.notes.dtype == torch.float32
    assert np.array_equal(_bits(s.notes.numpy()), _bits(MAJOR)), "feature_retrieval.note_table and the helper's disagree"
    assert float(s.notes[0]) == float(H.midi_hz(24)) and float(s.notes[42]) == float(H.midi_hz(96)) and bool(torch.isinf(s.notes[43:]).all())
    assert s.params() == tuple(float(v) for v in H.settings(MAJOR, N_MAJOR))
    assert s.f_min == 32.0 and abs(s.f_max - 2093.0 * 2 ** (1 / 12)) < 0.1
    assert PitchSnap(scale="chromatic").n_notes == 73 and PitchSnap(scale="pentatonic", key="F#").n_notes == 30
    assert PitchSnap(retune_ms=0).retune == 1.0 and PitchSnap(hysteresis_cents=0).hysteresis == 1.0
    assert PitchSnap(hysteresis_cents=100).hysteresis == float(F(2 ** (1 / 12)))
    for key, scale in (("A", "minor"), ("Eb", "major"), ("C", "chromatic")):
        assert np.array_equal(_bits(PitchSnap(key, scale).notes.numpy()), _bits(H.note_table(key, scale)[0]))
    e = PitchSnap(notes=[69, 57, 60, 69], a4=442.0)
    assert e.n_notes == 3 and float(e.notes[2]) == float(F(442.0)) and e.f_max == float(F(442.0 * 2 ** (1 / 12)))
    st = s.settings()
    assert isinstance(st, _lib.PitchSnapSettings) and (st.hysteresis, st.retune, st.f_min, st.f_max) == s.params()
    where = s.notes.data_ptr()
    s.set_scale("A", "minor")
    assert s.notes.data_ptr() == where and np.array_equal(_bits(s.notes.numpy()), _bits(H.note_table("A", "minor")[0]))
    s.bind(torch.device("cpu"), 3)
    assert s.strength.tolist() == [1.0, 1.0, 1.0] and s.notes.data_ptr() == where
    p = PitchSnap(strength=[0.25, 1.0]).bind(torch.device("cpu"), 2)
    assert p.strength.tolist() == [0.25, 1.0]
    with pytest.raises(ValueError, match="2 strengths for 3 rows"):
        p.bind(torch.device("cpu"), 3)


@pytest.mark.parametrize("kw", [
    dict(key="H"), dict(scale="dorian"), dict(notes=[]), dict(notes=[60.5]), dict(notes=[128]), dict(notes="60"), dict(notes=[True]), dict(a4=0.0),
    dict(a4=float("nan")), dict(a4=float("inf")), dict(a4="440"), dict(low=-1), dict(high=128), dict(low=70, high=60), dict(low=61, high=61, key="C"),
    dict(retune_ms=-1.0), dict(retune_ms=float("inf")), dict(retune_ms=float("nan")), dict(retune_ms=1e30), dict(strength=1.5), dict(strength=-0.1),
    dict(strength=float("nan")), dict(strength=[]), dict(strength=[0.5, 2.0]), dict(strength="1"), dict(hysteresis_cents=-1.0), dict(hysteresis_cents=101.0),
    dict(hysteresis_cents=float("nan")), dict(a4=1e-40), dict(a4=1e38), dict(notes=[0], a4=20.0)])
def test_every_refusal_comes_before_any_engine_work(kw, monkeypatch):
    monkeypatch.setattr(FR, "default_engine", lambda *a, **k: pytest.fail("engine work before the refusal"))
    with pytest.raises(ValueError, match="tune"):
        PitchSnap(**kw)


def test_parsing_and_resolving():
    assert FR.parse_tune("A minor") == ("A", "minor") and FR.parse_tune("chromatic") == ("C", "chromatic") and FR.parse_tune("F#") == ("F#", "major")
    assert FR.parse_tune("  Bb   pentatonic ") == ("Bb", "pentatonic")
    for bad in ("", "minor A", "A minor 7", "a minor", "C Major", None, 5):
        with pytest.raises(ValueError, match="tune"):
            FR.parse_tune(bad)
    s = FR.resolve_tune("A minor")
    assert isinstance(s, PitchSnap) and np.array_equal(_bits(s.notes.numpy()), _bits(H.note_table("A", "minor")[0]))
    assert FR.resolve_tune(None) is None and FR.resolve_tune(s) is s
    with pytest.raises(ValueError, match="tune"):
        FR.resolve_tune(3.0)
    with pytest.raises(ValueError, match="whole number of 480-sample frames"):
        FR.check_stream_tune("C major", 2000)
    assert FR.check_stream_tune(None, 2000) is None and isinstance(FR.check_stream_tune("C major", 1920), PitchSnap)


def test_snap_carry_and_its_state_table():
    names = [(f.name, f.dtype, f.tail, f.start) for f in stream_state.SNAP_STATE]
    assert names == [("note", torch.int32, (), -1), ("ratio", torch.float32, (), 1.0)]
    c = SnapCarry(3, 4, device="cpu")
    assert c.params() == (4,) and c.note.tolist() == [-1] * 3 and c.ratio.tolist() == [1.0] * 3
    c.note.copy_(torch.tensor([5, 6, 7], dtype=torch.int32))
    c.ratio.fill_(1.25)
    where = (c.note.data_ptr(), c.ratio.data_ptr())
    c.reset([1])
    assert c.note.tolist() == [5, -1, 7] and c.ratio.tolist() == [1.25, 1.0, 1.25] and stream_state.addresses(c, stream_state.SNAP_STATE) == where
    assert [t.data_ptr() for t in stream_state.checked(c, stream_state.SNAP_STATE, 3, torch.device("cpu"), "tune_carry.")] == list(where)
    c.reset()
    assert c.note.tolist() == [-1] * 3 and c.ratio.tolist() == [1.0] * 3
    c.ratio = torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="tune_carry.ratio"):
        stream_state.checked(c, stream_state.SNAP_STATE, 3, torch.device("cpu"), "tune_carry.")
    for bad in ((0, 4), (3, 0), (True, 4), (3, 4.0), (2 ** 31, 4)):
        with pytest.raises(ValueError, match="SnapCarry"):
            SnapCarry(*bad, device="cpu")
    ok = SnapCarry(2, 4, device="cpu")
    assert FR.check_tune_carry(ok, PitchSnap(), 2, 28) is ok and FR.check_tune_carry(None, None, 2, 28) is None
    for args, why in (((ok, None, 2, 28), "needs tune"), ((ok, PitchSnap(), 3, 28), "a carry of 2 streams"), ((ok, PitchSnap(), 2, 3), "hop_frames"),
                      ((object(), PitchSnap(), 2, 28), "SnapCarry")):
        with pytest.raises(ValueError, match=why):
            FR.check_tune_carry(*args)


def test_the_entry_scripts_flags():
    import infer
    import infer_streaming
    for mod in (infer, infer_streaming):
        a = mod.build_parser().parse_args(["--tune", "A minor", "--tune-a4", "442", "--tune-retune", "30", "--tune-strength", "0.5", "--tune-hysteresis", "10"])
        snap = FR.tune_keywords(a, "x.py")["tune"]
        want = PitchSnap("A", "minor", a4=442.0, retune_ms=30.0, strength=0.5, hysteresis_cents=10.0)
        assert snap.params() == want.params() and torch.equal(snap.notes, want.notes) and snap.strength.tolist() == [0.5]
        assert FR.tune_keywords(mod.build_parser().parse_args([]), "x.py") == {}
        a = mod.build_parser().parse_args(["--tune-notes", "57,60,64"])
        assert FR.tune_keywords(a, "x.py")["tune"].n_notes == 3
        for argv in (["--tune-retune", "30"], ["--tune", "H minor"], ["--tune", "C major", "--tune-strength", "2"], ["--tune-notes", "a,b"],
                     ["--tune", "C major", "--tune-notes", "60"]):
            with pytest.raises(SystemExit, match="x.py: "):
                FR.tune_keywords(mod.build_parser().parse_args(argv), "x.py")
    p = argparse.ArgumentParser()
    FR.add_tune_arguments(p)
    assert {a.dest for a in p._actions} >= {"tune", "tune_notes", "tune_a4", "tune_retune", "tune_strength", "tune_hysteresis"}


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_prototypes_are_declared_as_the_header_has_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    for name in ("tvc_pitch_snap_f32", "tvc_tuned_convert_f32", "tvc_tuned_convert_ragged_f32"):
        assert name in protos and name in _lib.PROTOTYPES, name
        names = [re.findall(r"[A-Za-z_]\w*", a)[-1] for a in protos[name].split(",")]
        assert [n for n, _t in _lib.PROTOTYPES[name][1]] == names, name
        assert not re.fullmatch(r"tvc_convert\w*_f32", name)
    tuned = [n for n, _t in _lib.PROTOTYPES["tvc_tuned_convert_f32"][1]]
    carry = [n for n, _t in _lib.PROTOTYPES["tvc_convert_carry_f32"][1]]
    extra = ["snap", "notes", "strength", "snap_carry_frame", "snap_note", "snap_ratio"]
    assert [n for n in tuned if n not in extra] == carry and [n for n in tuned if n in extra] == extra
    ragged = [n for n, _t in _lib.PROTOTYPES["tvc_tuned_convert_ragged_f32"][1]]
    assert [n for n in ragged if n not in extra] == [n for n, _t in _lib.PROTOTYPES["tvc_convert_ragged_path_f32"][1]] and [n for n in ragged if n in extra] == extra[:3]
    assert "typedef struct tvc_pitch_snap" in src and [f for f, _t in _lib.PitchSnapSettings._fields_] == ["hysteresis", "retune", "f_min", "f_max"]
    from tinyvc_amd import build
    assert "pitch_snap.hip" in build.SOURCES
