"""Pitch correction on the device (tvc_pitch_snap_f32, tvc_tuned_convert_f32 / tvc_tuned_convert_ragged_f32; Engine.pitch_snap,
Generator.convert(tune=, tune_carry=), BatchedStreamInfer(tune=), --tune in both entry scripts).

Contract (include/tinyvc_hip.h, restated in tests/helpers_pitch_snap.py): out, note_out and the carried state equal the numpy fp32
restatement BIT FOR BIT - every operation is one correctly rounded fp32 operation or an exact compare, so there is no tolerance anywhere in
this file.  Rows of every length around the 64-frame chunk, equal rows in one launch and row tables past the 256-row launch, in place and
out of place; tables a caller broke; states a caller scribbled into.  The fused conversion equals its stage composition bit for bit, a
strength of 0 and tune=None are today's call, a captured stream graph follows the table, the strengths and a reset.  Nobody has listened."""
import numpy as np
import pytest
import torch

import helpers_pitch_snap as H
import helpers_workspace as W
from helpers import state_dicts
from tinyvc_amd import audio_io, synth
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath, PitchSnap, SnapCarry, prepare_references

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
STRENGTHS = [0.0, 1.0, 0.5, np.nan, 7.0]


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.fixture(scope="module")
def targets():
    return [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------
def _tables():
    chromatic, n = H.note_table(scale="chromatic")
    assert n == 73
    single = np.full(128, np.inf, F)
    single[0] = 220.0
    full = np.array([H.midi_hz(30 + 0.5 * i) for i in range(128)], dtype=F)      # quarter tones: exactly 128 notes, none +inf
    broken = chromatic.copy()
    broken[40] = broken[38]                                                        # not ascending at 40: K = 40
    holed = chromatic.copy()
    holed[17] = np.nan                                                             # K = 17
    nothing = np.full(128, np.inf, F)                                              # K = 0
    return {"chromatic": chromatic, "single": single, "full128": full, "broken": broken, "nan": holed, "all_inf": nothing}


TABLES = _tables()


def _settings(table, cents=25.0, retune_ms=60.0):
    K = H.table_size(table)
    if K == 0:
        return F(2.0 ** (cents / 1200.0)), F(0.2834687), F(32.0), F(2217.4612)
    return H.settings(table, K, retune_ms, cents)


def _tune(table, settings, strengths):
    """a PitchSnap carrying exactly this table, these host values and these strengths, bound to the device"""
    t = PitchSnap(scale="chromatic")
    t.hysteresis, t.retune, t.f_min, t.f_max = (float(x) for x in settings)
    t.bind(torch.device(DEV), len(strengths))
    t.notes.copy_(_dev(np.asarray(table, dtype=F)))
    t.strength.copy_(_dev(np.asarray(strengths, dtype=F)))
    return t


# ---- contents ----------------------------------------------------------------------------------------------------------------------------------
def _content(n, seed, table, settings):
    """n frames: a melody that wanders in steps of a few cents (so a note is held, left and re-entered), random leaps between 40 and
    1500 Hz, unvoiced stretches, and the special values - 0, negatives, NaN, +-inf, and frames exactly on b[i], lo[i], hi[i], f_min and
    f_max and one ulp to either side of them"""
    r = np.random.default_rng(seed)
    h, _g, f_min, f_max = settings
    K, b, lo, hi = H.bounds(table, h)
    x = np.empty(n, dtype=np.float64)
    f = float(np.exp(r.uniform(np.log(40.0), np.log(1500.0))))
    for t in range(n):
        u = r.random()
        if u < 0.08:
            f = float(np.exp(r.uniform(np.log(40.0), np.log(1500.0))))
        else:
            f *= 2.0 ** (r.normal(0.0, 12.0) / 1200.0)
        f = min(max(f, 35.0), 1800.0)
        x[t] = f
    x = x.astype(F)
    t = 0
    while t < n:      # unvoiced stretches
        if r.random() < 0.04:
            k = int(r.integers(1, 9))
            x[t:t + k] = 0
            t += k
        t += 1
    edges = [v for v in np.concatenate([b, lo[1:], hi[:-1], [f_min, f_max]]) if np.isfinite(v)]
    exact = []
    for v in edges:
        v = F(v)
        exact += [v, np.nextafter(v, F(0)), np.nextafter(v, F(np.inf))]
    special = [F(0), F(-0.0), F(-100), F(np.nan), F(np.inf), F(-np.inf), F(31.999), F(1e-30), F(3e38)] + exact
    where = r.choice(n, size=min(n, max(1, n // 3)), replace=False)
    for i in where:
        x[i] = special[int(r.integers(0, len(special)))]
    return x


def _check(eng, f0, starts, counts, table, settings, strengths, what, state=None, hop=0):
    """the stage call in place and out of place against the helper: out, note_out and the state, bit for bit"""
    rows = len(starts)
    tune = _tune(table, settings, strengths)
    want_out, want_note, want_state = H.snap_rows(f0, starts, counts, table, *settings, strength=strengths, state=state, carry_frame=hop)
    want_note = np.where(want_note == -7, -1, want_note)      # columns outside every row: the engine's note_out starts at -1
    got = []
    for in_place in (False, True):
        carry = None
        if state is not None:
            carry = SnapCarry(rows, hop, device=DEV)
            carry.note.copy_(_dev(np.asarray(state[0], dtype=np.int32)))
            carry.ratio.copy_(_dev(np.asarray(state[1], dtype=F)))
        x = _dev(f0)
        out, note = eng.pitch_snap(x, tune, row_start=starts, row_count=counts, carry=carry, in_place=in_place)
        assert (out.data_ptr() == x.data_ptr()) == in_place
        got.append((out.cpu().numpy(), note.cpu().numpy(), None if carry is None else (carry.note.cpu().numpy(), carry.ratio.cpu().numpy())))
    for (out, note, st), mode in zip(got, ("out of place", "in place")):
        bad = np.nonzero(_bits(out) != _bits(want_out))[0]
        assert not len(bad), f"{what} ({mode}): out differs at {bad[:8]}: {out[bad[:4]]} against {want_out[bad[:4]]} for f0 {f0[bad[:4]]}"
        bad = np.nonzero(note != want_note)[0]
        assert not len(bad), f"{what} ({mode}): note_out differs at {bad[:8]}: {note[bad[:4]]} against {want_note[bad[:4]]}"
        if state is not None:
            assert np.array_equal(st[0], want_state[0]), f"{what} ({mode}): the carried notes {st[0][:8]} against {want_state[0][:8]}"
            assert np.array_equal(_bits(st[1]), _bits(want_state[1])), f"{what} ({mode}): the carried ratios"
    return want_out, want_note


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 200])
def test_equal_rows_around_the_chunk(gen, T):
    R, table = 5, TABLES["chromatic"]
    s = _settings(table)
    f0 = np.concatenate([_content(T, 100 * T + b, table, s) for b in range(R)])
    out, note = _check(gen.engine(), f0, [b * T for b in range(R)], [T] * R, table, s, STRENGTHS, f"{R} rows of {T}")
    if T >= 63:
        assert (note >= 0).sum() > T and (note < 0).sum() > 0 and not np.array_equal(_bits(out), _bits(f0)), "the case shows nothing"


def test_257_equal_rows_with_state(gen):
    R, T, hop, table = 257, 65, 64, TABLES["chromatic"]
    s = _settings(table)
    f0 = np.concatenate([_content(T, 7000 + b, table, s) for b in range(R)])
    r = np.random.default_rng(9)
    state = (r.integers(-1, 73, R).astype(np.int32), r.uniform(0.9, 1.1, R).astype(F))
    strengths = [STRENGTHS[b % 5] for b in range(R)]
    _check(gen.engine(), f0, [b * T for b in range(R)], [T] * R, table, s, strengths, "257 rows", state=state, hop=hop)


def test_a_row_table_with_an_empty_row_gaps_and_odd_starts(gen):
    table = TABLES["chromatic"]
    s = _settings(table)
    starts, counts = [3, 10, 80, 81, 300, 517], [1, 63, 0, 129, 200, 65]
    f0 = _content(600, 31, table, s)
    out, note = _check(gen.engine(), f0, starts, counts, table, s, [1.0, 0.5, 1.0, 7.0, np.nan, 1.0], "ragged rows")
    outside = np.ones(600, bool)
    for a, n in zip(starts, counts):
        outside[a:a + n] = False
    assert np.array_equal(_bits(out[outside]), _bits(f0[outside])) and (note[outside] == -1).all()
    # with a state: hop 1 is the only one every non-empty row has
    state = (np.array([5, 1000, 3, -5, 20, 40], np.int32), np.array([1.01, 1.0, 0.5, 1.0, np.nan, 9.0], F))
    _check(gen.engine(), f0, starts, counts, table, s, [1.0] * 6, "ragged rows with a state", state=state, hop=1)


def test_a_row_table_past_the_256_row_launch(gen):
    table = TABLES["chromatic"]
    s = _settings(table)
    r = np.random.default_rng(77)
    counts = [int(c) for c in r.integers(1, 6, 300)]
    starts = [int(a) for a in np.cumsum([2] + [c + int(g) for c, g in zip(counts[:-1], r.integers(0, 3, 299))])]
    f0 = _content(starts[-1] + counts[-1] + 5, 78, table, s)
    state = (r.integers(-1, 73, 300).astype(np.int32), r.uniform(0.7, 1.4, 300).astype(F))
    _check(gen.engine(), f0, starts, counts, table, s, [STRENGTHS[b % 5] for b in range(300)], "300 ragged rows", state=state, hop=1)


# ---- 2. tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("cents", [0.0, 25.0, 100.0])
def test_tables(gen, name, cents):
    table = TABLES[name]
    assert H.table_size(table) == {"chromatic": 73, "single": 1, "full128": 128, "broken": 40, "nan": 17, "all_inf": 0}[name]
    s = _settings(table, cents, retune_ms=0.0 if cents == 0.0 else 60.0)
    R, T = 3, 200
    f0 = np.concatenate([_content(T, 900 + 10 * b + int(cents), table, s) for b in range(R)])
    out, note = _check(gen.engine(), f0, [b * T for b in range(R)], [T] * R, table, s, [1.0, 0.5, 1.0], f"table {name} at {cents} cents")
    if name == "all_inf":
        assert np.array_equal(_bits(out), _bits(f0)) and (note == -1).all(), "K = 0 must return the input bits"
    else:
        assert note.max() < H.table_size(table) and (note >= 0).any()
        assert (out[note >= 0] > 20).all(), "a corrected frame under the decoder's voicing gate"


# ---- 3. the state ------------------------------------------------------------------------------------------------------------------------------
def test_carried_windows_over_six_blocks_with_a_reset(gen):
    eng, R, T, hop, nwin, table = gen.engine(), 3, 28, 4, 6, TABLES["chromatic"]
    s = _settings(table)
    total = (nwin - 1) * hop + T
    x = np.stack([_content(total, 500 + b, table, s) for b in range(R)])
    tune = _tune(table, s, [1.0, 0.5, 1.0])
    carry = SnapCarry(R, hop, device=DEV)
    state = (np.full(R, -1, np.int32), np.ones(R, F))
    for n in range(nwin):
        if n == 3:      # between blocks: stream 1 starts without a note, in place
            carry.reset([1])
            state[0][1], state[1][1] = -1, 1.0
        win = np.ascontiguousarray(x[:, n * hop:n * hop + T])
        out, note = eng.pitch_snap(_dev(win), tune, carry=carry)
        w_out, w_note, state = H.snap_rows(win.reshape(-1), [b * T for b in range(R)], [T] * R, table, *s, strength=[1.0, 0.5, 1.0], state=state, carry_frame=hop)
        assert np.array_equal(_bits(out.cpu().numpy().reshape(-1)), _bits(w_out)) and np.array_equal(note.cpu().numpy().reshape(-1), w_note), f"window {n}"
        assert np.array_equal(carry.note.cpu().numpy(), state[0]) and np.array_equal(_bits(carry.ratio.cpu().numpy()), _bits(state[1])), f"window {n}: the state"
        if n < 3:      # up to the reset the windows are the run over the whole prefix
            for b in range(R):
                p_out, p_note, _ = H.snap_row(x[b, :n * hop + T], table, *s, strength=[1.0, 0.5, 1.0][b])
                assert np.array_equal(_bits(out[b].cpu().numpy()), _bits(p_out[n * hop:])) and np.array_equal(note[b].cpu().numpy(), p_note[n * hop:])


def test_garbage_states_count_as_none(gen):
    table = TABLES["chromatic"]
    s = _settings(table)
    notes = np.array([1000, -5, 10, 10, 73, 72, 0, -1, 2 ** 31 - 1, -2 ** 31], np.int32)
    ratios = np.array([1.0, 1.0, np.nan, 9.0, 1.0, 1.5, H.RATIO_MIN, 1.0, np.inf, 0.0], F)
    R, T = len(notes), 30
    f0 = np.concatenate([_content(T, 40 + b, table, s) for b in range(R)])
    f0[::T] = [H.midi_hz(34 + 3 * b) * F(1.004) for b in range(R)]      # every row starts in range, near a note: a valid prior would matter
    _check(gen.engine(), f0, [b * T for b in range(R)], [T] * R, table, s, [1.0] * R, "garbage states", state=(notes, ratios), hop=T)


def test_refusals(gen):
    eng = gen.engine()
    tune = PitchSnap()
    f0 = torch.zeros(2, 28, device=DEV)
    with pytest.raises(ValueError, match="hop_frames"):
        eng.pitch_snap(f0, tune, carry=SnapCarry(2, 29, device=DEV))
    with pytest.raises(ValueError, match="a carry of 3 streams"):
        eng.pitch_snap(f0, tune, carry=SnapCarry(3, 4, device=DEV))
    for name, value in (("hysteresis", 0.99), ("hysteresis", 1.06), ("retune", 0.0), ("retune", 1.5), ("f_min", 31.0), ("f_max", float("inf")), ("f_max", 10.0)):
        bad = PitchSnap()
        setattr(bad, name, value)
        with pytest.raises(Exception, match="snap: "):
            eng.pitch_snap(f0, bad)
    wf, tg = torch.zeros(2, 28 * 480, device=DEV), synth.synth_index(300, seed=21).to(DEV)
    with pytest.raises(ValueError, match="tune_carry"):
        gen.convert(wf, tg, 0.0, tune="C major", tune_carry=SnapCarry(3, 4, device=DEV))
    with pytest.raises(ValueError, match="tune_carry"):
        gen.convert(wf, tg, 0.0, tune_carry=SnapCarry(2, 4, device=DEV))
    with pytest.raises(ValueError, match="no ragged form"):
        gen.convert(wf, tg, 0.0, tune="C major", tune_carry=SnapCarry(2, 4, device=DEV), lengths=[28 * 480, 480 * 20])


# ---- 4. the fused conversion -------------------------------------------------------------------------------------------------------------------
B2, T2 = 2, 28
SHIFTS2 = [2.0, -3.0]
PATH2 = PitchPath(0.5, 12, 12.0, 1.0, 2)


def _stages(gen, wf):
    from tinyvc_amd.module import utils
    eng = gen.engine()
    w = utils.autopad_waveform(wf.to(DEV))
    ssl, f0, logits = eng.encoder(utils.spectrogram(w), want_logits=True)
    return eng, ssl, f0, logits, utils.estimate_energy(w)


def _tuned(strength=(1.0, 0.5)):
    return PitchSnap(scale="chromatic", low=12, retune_ms=40.0, strength=list(strength))


@pytest.mark.parametrize("case", ["plain", "viterbi", "auto_pitch", "alpha_protect"])
def test_convert_equals_its_stage_composition(gen, targets, case):
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, f0, logits, energy = _stages(gen, wf)
    blobs, ns = prepare_references(targets)
    kw, matched = {}, None
    if case == "plain":
        f0s = eng.pitch_match(f0, pitch_shift=SHIFTS2, want_shifted=True)[3]
    else:
        kw["f0_estimation"] = PATH2
        f0, _p, _sc, f0s = eng.pitch_path(logits, PATH2, pitch_shift=SHIFTS2, want_shifted=True)
    if case == "auto_pitch":
        kw["auto_pitch"] = reg = torch.tensor([180.0, 240.0], device=DEV)
        f0s = eng.pitch_match(f0, target_f0=reg, pitch_shift=SHIFTS2, want_shifted=True)[3]
    if case == "alpha_protect":
        kw["alpha"], kw["protect"] = torch.tensor([0.3, 0.0], device=DEV), torch.tensor([0.5, 1.0], device=DEV)
        matched = eng.knn_match_protect(ssl, f0, blobs, ns, kw["alpha"], kw["protect"])      # protect reads the f0 in front of the correction
    if matched is None:
        matched = eng.knn_match_multi(ssl, blobs, ns)
    today = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, **kw)
    assert torch.equal(today, eng.decoder(matched, f0s, energy, angle)), f"{case}: the composition is not today's call: the comparison shows nothing"
    tune = _tuned()
    out = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, tune=tune, **kw)
    snapped, note = eng.pitch_snap(f0s, tune)
    assert int((note >= 0).sum()) > T2 // 2, f"{case}: hardly a frame of this f0 is in range: the case shows nothing"
    assert torch.equal(out, eng.decoder(matched, snapped, energy, angle)), f"{case}: convert(tune=) != the stages, pitch_snap, the decoder"
    assert not torch.equal(out, today), f"{case}: the correction changed nothing"
    # tune=None and a strength of 0 are today's call, bit for bit
    assert torch.equal(gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, tune=None, **kw), today)
    assert torch.equal(gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, tune=_tuned((0.0, 0.0)), **kw), today), f"{case}: strength 0"
    # a row equals its own call, with its own strength
    for b in range(B2):
        one = {k: (v[b:b + 1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        y = gen.convert(wf[b:b + 1].to(DEV), targets[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), tune=_tuned((1.0, 0.5)[b:b + 1]), **one)
        assert torch.equal(out[b:b + 1], y), f"{case}: row {b} != its own call"


def test_convert_with_a_state_equals_the_composition(gen, targets):
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, f0, _logits, energy = _stages(gen, wf)
    blobs, ns = prepare_references(targets)
    f0s = eng.pitch_match(f0, pitch_shift=SHIFTS2, want_shifted=True)[3]
    tune = _tuned()
    first = eng.pitch_snap(f0s, tune)[1][:, 0, 0].cpu().numpy()
    mine, theirs = SnapCarry(B2, 4, device=DEV), SnapCarry(B2, 4, device=DEV)
    for c in (mine, theirs):      # a note beside the one the first frame would pick, and a ratio away from 1
        c.note.copy_(_dev(np.maximum(first, 0).astype(np.int32) + 1))
        c.ratio.fill_(1.2)
    where = mine.note.data_ptr()
    out = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, tune=tune, tune_carry=mine)
    snapped, _n = eng.pitch_snap(f0s, tune, carry=theirs)
    assert torch.equal(out, eng.decoder(eng.knn_match_multi(ssl, blobs, ns), snapped, energy, angle))
    assert torch.equal(mine.note, theirs.note) and torch.equal(mine.ratio, theirs.ratio) and mine.note.data_ptr() == where
    assert not torch.equal(out, gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, tune=tune)), "the prior changed nothing"


@pytest.mark.parametrize("viterbi", [False, True])
def test_ragged_convert_equals_each_rows_composition(gen, targets, viterbi):
    frames, B = [28, 13, 7], 3
    Tmax, lens = max(frames), [f * 480 for f in frames]
    wf = synth.synth_wave(B, Tmax * 480, seed=51)
    for b, f in enumerate(frames):
        wf[b, f * 480:] = 0
    tg = [targets[0], targets[1], targets[0]]
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    kw = {"f0_estimation": PATH2} if viterbi else {}
    strengths = [1.0, 0.5, 0.8]
    out = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, tune=_tuned(strengths), **kw)
    today = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, **kw)
    assert torch.equal(gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, tune=_tuned([0.0] * 3), **kw), today), "strength 0"
    assert not torch.equal(out, today)
    blobs, ns = prepare_references(tg)
    for b, f in enumerate(frames):
        eng, ssl, f0, logits, energy = _stages(gen, wf[b:b + 1, :lens[b]])
        f0s = eng.pitch_path(logits, PATH2, pitch_shift=-2.0, want_shifted=True)[3] if viterbi else eng.shift_frequency(f0, -2.0)
        snapped, _n = eng.pitch_snap(f0s, _tuned(strengths[b:b + 1]))
        want = eng.decoder(eng.knn_match_multi(ssl, blobs[b:b + 1], ns[b:b + 1]), snapped, energy, angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b:b + 1, :lens[b]], want), f"row {b} of {f} frames"
        assert not out[b, lens[b]:].any()


# ---- 5. streams --------------------------------------------------------------------------------------------------------------------------------
def test_streams(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk, shifts = 3, 6, [0.0, 3.0, -2.0]
    tg = [targets[0], targets[1], targets[0]]
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)

    def make(use_graph, tuned):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=shifts, device=torch.device(DEV), use_graph=use_graph,
                                tune=PitchSnap(scale="chromatic", low=12, retune_ms=40.0) if tuned else None)
        st.init_buffer()
        return st

    graph, eager, plain = make(True, True), make(False, True), make(False, False)
    assert eager.tune_carry.params() == (4,) and plain.tune is None and plain.tune_carry is None
    assert [name for name, _s, _t in eager._stages()] == ["tune_carry"] and plain._stages() == []
    eng = gen.engine()
    window = torch.zeros(S, eager.input_size, device=DEV)
    own_tune, own = PitchSnap(scale="chromatic", low=12, retune_ms=40.0), SnapCarry(S, 4, device=DEV)
    sola, sola_plain = torch.zeros(S, eager.crossfade_size, device=DEV), torch.zeros(S, eager.crossfade_size, device=DEV)
    minor = _dev(np.asarray(H.note_table("A", "minor", low=12)[0], dtype=F))

    def tail(y, buf):
        return eng.sola(y, buf, eager.fade_in_window, 1920, False, want_shift=True, crossfade=eager.crossfade_size, search=eager.sola_search_size,
                        delay=eager.last_dilay_size)[0]

    captured = None
    for i in range(nblk):
        angle = synth.synth_angle(S, 28, 850 + i).to(DEV)
        if i == 3:      # between replays, all in place: another table, other strengths, stream 1 without a note
            for st_tune, st_carry in ((graph.tune, graph.tune_carry), (eager.tune, eager.tune_carry), (own_tune.bind(torch.device(DEV), S), own)):
                st_tune.notes.copy_(minor)
                st_tune.strength.fill_(0.5)
                st_carry.reset([1])
        a, b, p = (st.audio_callback(blocks[:, i], noise_angle=angle).clone() for st in (graph, eager, plain))
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(graph.tune_carry.note, eager.tune_carry.note) and torch.equal(graph.tune_carry.ratio, eager.tune_carry.ratio), f"block {i + 1}: the state"
        window = torch.cat([window[:, 1920:], blocks[:, i]], dim=1).contiguous()
        y = gen.convert(window, tg, shifts, noise_angle=angle, tune=own_tune, tune_carry=own)
        assert torch.equal(b, tail(y, sola)), f"block {i + 1} != convert(window, tune=, tune_carry=) through the tail"
        assert torch.equal(own.note, eager.tune_carry.note) and torch.equal(own.ratio, eager.tune_carry.ratio)
        if i == 2:
            captured = graph._graph[1][True][0]      # captured at block 3
            key = graph._graph_key()
        if i > 2:
            assert graph._graph[1][True][0] is captured and graph._graph_key() == key, "a new table, new strengths or a reset must keep the graph"
        # a stream without tune is the stream as it was: the plain convert of its window through the tail
        assert torch.equal(p, tail(gen.convert(window, tg, shifts, noise_angle=angle), sola_plain)), f"block {i + 1}: tune=None"
    assert not torch.equal(a, p), "the correction changed nothing in six blocks: the comparison shows nothing"
    graph.tune.retune = 0.5
    assert graph._graph_key() != key, "retune is baked into the launch: another value must be another key"
    with pytest.raises(ValueError, match="whole number of 480-sample frames"):
        BatchedStreamInfer(gen, n_streams=1, target=tg[0], device=torch.device(DEV), block_size=2000, tune="C major")


# ---- 6. the tuned entries in a poisoned, guarded workspace of exactly their peak ------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_tuned_entries_in_a_poisoned_workspace(gen, ragged):
    eng = gen.engine()
    T, frames = 37, [37, 13, 7]
    rows = 3 if ragged else 2
    wav = synth.synth_wave(rows, T * 480, seed=611)
    if ragged:
        for b, f in enumerate(frames):
            wav[b, f * 480:] = 0
    wav, angle = wav.to(DEV), synth.synth_angle(rows, T, 612).to(DEV)
    lens = [f * 480 for f in frames] if ragged else None
    small, big = eng.knn_prepare(synth.synth_index(129, seed=615).to(DEV)), eng.knn_prepare(synth.synth_index(4097, seed=616).to(DEV).half())
    prepared, ns = [(small, big)[r % 2][0] for r in range(rows)], [(small, big)[r % 2][1] for r in range(rows)]
    shifts, target = [2.0, -3.0, 1.0][:rows], _dev(np.array([150.0, 220.0, 180.0][:rows], F))
    alpha, protect = _dev(np.array([0.25, 0.6, 0.0][:rows], F)), _dev(np.array([0.5, 1.0, 0.75][:rows], F))
    tune = _tuned([1.0, 0.5, 0.8][:rows])

    def call(_outs=None):
        carry = None
        if not ragged:
            carry = SnapCarry(rows, 4, device=DEV)
            carry.note.fill_(30)
            carry.ratio.fill_(1.1)
        res = eng._convert("tuned", wav, prepared, ns, shifts, angle, lens, None, target, alpha=alpha, protect=protect, path=PitchPath(), tune=tune, tune_carry=carry)
        return (res, carry.note, carry.ratio) if carry is not None else res

    want = call()
    torch.cuda.synchronize()
    if ragged:
        eng.set_ragged_batch_frames(45)
    try:
        if ragged:
            want = call()
        for word, phase in zip(W.FILLS, W.PHASES):
            with W.guarded_workspace(eng, word, phase) as g:
                got = call()
            W.assert_same_bits(got, want, f"tuned {'ragged' if ragged else 'equal'} under fill {word:#010x} at phase {phase}")
            assert g.peaks and all(p > 0 for p in g.peaks)
    finally:
        eng.set_ragged_batch_frames(0)


# ---- 7. the entry scripts ------------------------------------------------------------------------------------------------------------------------
def test_entry_scripts(tmp_path, capsys):
    import infer
    import infer_streaming
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(300, seed=2), d / "a.pt")
    (d / "inputs").mkdir()
    audio_io.save(str(d / "inputs" / "x.wav"), synth.synth_wave(1, 12000, seed=3) * 0.9, 24000)
    common = ["-i", str(d / "inputs"), "-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "a.pt"), "-p", "1.0", "-d", DEV, "--seed", "3"]
    assert infer.main(common + ["-o", str(d / "plain")]) == 0
    assert infer.main(common + ["-o", str(d / "tuned"), "--tune", "C major", "--tune-retune", "0"]) == 0
    assert "Correcting pitch" in capsys.readouterr().out
    plain, tuned = audio_io.load(str(d / "plain" / "x.wav"))[0], audio_io.load(str(d / "tuned" / "x.wav"))[0]
    assert plain.shape == tuned.shape and not torch.equal(plain, tuned), "--tune changed nothing"
    assert infer.main(common + ["-o", str(d / "chunked"), "--chunked", "-c", "1920", "--tune", "C major"]) == 0
    assert audio_io.load(str(d / "chunked" / "x.wav"))[0].shape == plain.shape
    audio_io.save(str(d / "mic.wav"), synth.synth_wave(1, 8 * 1920, seed=50) * 0.9, 24000)
    live = ["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "a.pt"), "--input-wav", str(d / "mic.wav"), "-d", DEV]
    torch.manual_seed(3)
    assert infer_streaming.main(live + ["--output-wav", str(d / "live_plain.wav")]) == 0
    torch.manual_seed(3)
    assert infer_streaming.main(live + ["--tune", "chromatic", "--tune-strength", "0.8", "--output-wav", str(d / "live_tuned.wav")]) == 0
    assert "Correcting pitch" in capsys.readouterr().out
    assert open(d / "live_plain.wav", "rb").read() != open(d / "live_tuned.wav", "rb").read(), "--tune changed nothing in the stream"
