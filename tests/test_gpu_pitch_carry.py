"""The pitch path's carry on the device (tvc_pitch_path_carry_f32, tvc_convert_carry_f32; Engine.pitch_path(prior=, carry_out=,
carry_frame=), Generator.convert(carry=PitchCarry), BatchedStreamInfer(f0_carry=)).

Contract (include/tinyvc_hip.h, restated in tests/helpers_pitch_carry.py on helpers_pitch_path): decoded window by window over slices of one
logits tensor, classes and the carried state equal the numpy fp32 restatement BIT FOR BIT, the last frame's scores by value, f0 within
helpers_pitch_path.f0_bound(refine) of the fp64 expectation - and every window equals the last T frames of the existing helper's decode of
the whole prefix.  In place equals out of place; carry_out alone is tvc_pitch_path_f32 bit for bit; row 256 takes element 256; whatever a
caller wrote into the state, the kernel decodes the sanitised one.  The fused conversion equals the stage composition bit for bit with the
same state afterwards; a captured stream graph follows the state, a reset included.  On planted logits the carried window stays on the
ridge the uncarried one leaves.  Nobody has listened."""
import ctypes
import math

import numpy as np
import pytest
import torch

import helpers_pitch_carry as C
import helpers_pitch_path as H
from helpers import state_dicts
from tinyvc_amd import synth
from tinyvc_amd.engine import pitch_class_table
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchCarry, PitchPath

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = math.inf
F = np.float32
SHAPES = [(12, 4), (5, 4), (6, 1), (28, 4)]      # (T, h)
NWIN = 6
INPUTS = {"gaussian": H.gaussian, "quantised": H.quantised, "special": H.special_columns}
ROWS = 2


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
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the stage call against the restatement, window by window ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}h{s[1]}")
@pytest.mark.parametrize("kind", list(INPUTS))
def test_windows_equal_the_helper_and_the_decode_of_the_prefix(gen, kind, shape):
    T, h = shape
    eng, s, freq = gen.engine(), H.DEFAULT, pitch_class_table().numpy()
    x = np.stack([INPUTS[kind]((NWIN - 1) * h + T, 31 * T + h + 100 * b) for b in range(ROWS)])
    want = [C.windows(x[b], s, T, h, NWIN) for b in range(ROWS)]
    state = torch.zeros(ROWS, 512, device=DEV)                                     # in place: prior is carry_out
    prior, out = torch.zeros(ROWS, 512, device=DEV), torch.zeros(ROWS, 512, device=DEV)      # out of place
    for n in range(NWIN):
        win = _dev(x[:, :, n * h:n * h + T])
        f0, path, scores = eng.pitch_path(win, PitchPath(*s), prior=state, carry_out=state, carry_frame=h)
        f0b, pathb, scoresb = eng.pitch_path(win, PitchPath(*s), prior=prior, carry_out=out, carry_frame=h)
        assert torch.equal(f0, f0b) and torch.equal(path, pathb) and torch.equal(scores, scoresb) and torch.equal(state, out), f"window {n}: in place"
        prior.copy_(out)
        f0, path, scores, carry = (t.cpu().numpy() for t in (f0, path, scores, state))
        for b in range(ROWS):
            wpath, _wbp, wsc, wcarry = want[b][n]
            what = f"{kind} {shape} window {n} row {b}"
            assert np.array_equal(path[b, 0], wpath), f"{what}: classes differ at frames {np.nonzero(path[b, 0] != wpath)[0][:8]}"
            assert np.array_equal(_bits(carry[b]), _bits(wcarry)), f"{what}: the carried state differs"
            assert np.array_equal(scores[b], wsc), f"{what}: the last frame's scores differ"
            end = n * h + T
            ppath, _pbp, psc = H.viterbi_banded(x[b][:, :end], s)
            assert np.array_equal(path[b, 0], ppath[end - T:]) and np.array_equal(scores[b], psc), f"{what} != the decode of the whole prefix"
            truth = H.frequency64(win[b].cpu().numpy(), wpath, s.refine, freq)
            err = np.abs(f0[b, 0].astype(np.float64) - truth)
            assert (err <= H.f0_bound(s.refine) * truth).all() and (f0[b, 0][wpath == 0] == 0).all(), f"{what}: f0"


def test_prior_alone_and_carry_out_alone(gen):
    eng, s, T, h = gen.engine(), PitchPath(), 12, 4
    x = np.stack([H.gaussian(T, 70), H.special_columns(T, 71)])
    win = _dev(x)
    plain = eng.pitch_path(win, s)
    out = torch.full((2, 512), 7.0, device=DEV)
    only_out = eng.pitch_path(win, s, carry_out=out, carry_frame=h)
    assert all(torch.equal(a, b) for a, b in zip(plain, only_out)), "carry_out alone changes tvc_pitch_path_f32's outputs"
    for b in range(2):
        assert np.array_equal(_bits(out[b].cpu().numpy()), _bits(C.viterbi_carried(x[b], H.DEFAULT, None, h)[3]))
    r = np.random.default_rng(3)
    p = (-4 * np.abs(r.standard_normal((2, 512)))).astype(F)
    prior = _dev(p)
    keep = prior.clone()
    _f0, path, scores = eng.pitch_path(win, s, prior=prior)      # carry_frame is not looked at without carry_out
    assert torch.equal(prior, keep), "prior alone was written"
    for b in range(2):
        wpath, _bp, wsc, _c = C.viterbi_carried(x[b], H.DEFAULT, p[b])
        assert np.array_equal(path[b, 0].cpu().numpy(), wpath) and np.array_equal(scores[b].cpu().numpy(), wsc)
    # a prior of zeros: the same classes, f0 and scores by value
    zero = eng.pitch_path(win, s, prior=torch.zeros(2, 512, device=DEV))
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]) and bool((zero[2] == plain[2]).all())


# ---- 2. rows: the 256-row launch boundary ---------------------------------------------------------------------------------------------------
def test_257_rows_each_with_its_own_prior(gen):
    eng, s, R, T, h = gen.engine(), PitchPath(), 257, 8, 3
    r = np.random.default_rng(12)
    x = _dev(r.standard_normal((R, 512, T)).astype(F))
    p = (-6 * np.abs(r.standard_normal((R, 512)))).astype(F)
    state = _dev(p)
    whole = eng.pitch_path(x, s, prior=state, carry_out=state, carry_frame=h)
    again_state = _dev(p)
    again = eng.pitch_path(x, s, prior=again_state, carry_out=again_state, carry_frame=h)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)) and torch.equal(state, again_state), "two runs differ"
    assert not torch.equal(state, _dev(p))
    for b in range(R):
        one_state = _dev(p[b:b + 1])
        one = eng.pitch_path(x[b:b + 1].contiguous(), s, prior=one_state, carry_out=one_state, carry_frame=h)
        assert all(torch.equal(w[b:b + 1], o) for w, o in zip(whole, one)) and torch.equal(state[b:b + 1], one_state), f"row {b} != the row alone"
    assert float(state.max(dim=1).values.abs().max()) == 0.0      # every row's carry has maximum exactly 0


# ---- 3. garbage states -----------------------------------------------------------------------------------------------------------------------
def test_garbage_states_decode_as_the_sanitised_state(gen):
    eng, s, T, h = gen.engine(), PitchPath(), 12, 4
    r = np.random.default_rng(5)
    mixed = (-3 * np.abs(r.standard_normal(512))).astype(F)
    mixed[r.integers(0, 512, 40)] = np.nan
    mixed[r.integers(0, 512, 40)] = INF
    mixed[r.integers(0, 512, 40)] = 2.5
    mixed[r.integers(0, 512, 40)] = -INF
    lone = np.full(512, -INF, F)
    lone[17] = np.nan                                      # NaN counts as 0 before the all -inf rule: class 17 alone is known
    states = np.stack([np.full(512, np.nan, F), np.full(512, INF, F), np.full(512, 3.0, F), np.full(512, -INF, F), mixed, lone])
    R = len(states)
    x = np.stack([H.gaussian(T, 90 + b) for b in range(R)])
    state = _dev(states)
    _f0, path, scores = eng.pitch_path(_dev(x), s, prior=state, carry_out=state, carry_frame=h)
    path, scores, carry = path.cpu().numpy(), scores.cpu().numpy(), state.cpu().numpy()
    for b in range(R):
        wpath, _bp, wsc, wcarry = C.viterbi_carried(x[b], H.DEFAULT, states[b], h)
        assert np.array_equal(path[b, 0], wpath) and np.array_equal(scores[b], wsc) and np.array_equal(_bits(carry[b]), _bits(wcarry)), f"state {b}"
        assert carry[b].max() == 0 and not np.isnan(carry[b]).any() and scores[b].max() == 0
    assert path[5, 0, 0] == 17


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(gen):
    from tinyvc_amd._lib import PitchPathSettings
    eng, s = gen.engine(), PitchPath()
    x = torch.zeros(2, 512, 8, device=DEV)
    state = torch.full((2, 512), -1.0, device=DEV)
    for h in (0, -1, 8, 9):      # carry_frame < 1; rows of <= h frames
        with pytest.raises(ValueError, match="carry_frame"):
            eng.pitch_path(x, s, prior=state, carry_out=state, carry_frame=h)
    for bad in (torch.zeros(3, 512, device=DEV), torch.zeros(2, 511, device=DEV), torch.zeros(2, 512, device=DEV, dtype=torch.float64),
                torch.zeros(2, 1024, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="contiguous fp32"):
            eng.pitch_path(x, s, prior=bad)
        with pytest.raises(ValueError, match="contiguous fp32"):
            eng.pitch_path(x, s, carry_out=bad, carry_frame=2)
    # the library's own host checks, before any device work
    I64 = ctypes.c_int64 * 2
    for h, counts in ((0, (8, 8)), (-3, (8, 8)), (8, (8, 8)), (4, (8, 4)), (4, (3, 8))):
        rc = eng.lib.tvc_pitch_path_carry_f32(eng.ctx, eng._stream(), x.data_ptr(), I64(0, 8), I64(*counts), 2, 8, ctypes.byref(PitchPathSettings(*s.params())), h,
                                              state.data_ptr(), state.data_ptr(), 0.0, None, None, None, None, None, None, 0)
        assert rc != 0 and b"carry_frame" in eng.lib.tvc_last_error(eng.ctx), (h, counts)
    torch.cuda.synchronize()
    assert (state == -1.0).all(), "a refused call wrote the state"
    # an empty row beside a long one is legal: it writes nothing, its state included
    eng.pitch_path(torch.zeros(512, 8, device=DEV), s, row_start=[0, 0, 8], prior=state, carry_out=state, carry_frame=4)
    assert (state[0] == -1.0).all() and float(state[1].max()) == 0.0
    # Engine._convert: the state against its table, the batch and the window
    wf = torch.zeros(2, 28 * 480, device=DEV)
    tg = synth.synth_index(300, seed=21).to(DEV)
    with pytest.raises(ValueError, match="a carry of 3 streams"):
        gen.convert(wf, tg, 0.0, f0_estimation=s, carry=PitchCarry(3, 4, device=DEV))
    with pytest.raises(ValueError, match="hop_frames"):
        gen.convert(wf, tg, 0.0, f0_estimation=s, carry=PitchCarry(2, 28, device=DEV))
    c = PitchCarry(2, 4, device=DEV)
    c.scores = torch.zeros(2, 256, device=DEV)
    with pytest.raises(ValueError, match="carry.scores"):
        gen.convert(wf, tg, 0.0, f0_estimation=s, carry=c)
    with pytest.raises(ValueError, match="form"):
        from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
        blobs, ns = prepare_references([tg, tg])
        eng._convert("table", wf, blobs, ns, 0.0, carry=PitchCarry(2, 4, device=DEV))


# ---- 5. the fused conversion -----------------------------------------------------------------------------------------------------------------
B2, T2, H2 = 2, 28, 4
SHIFTS2 = [2.0, -3.0]
SETTINGS2 = PitchPath(0.5, 12, 12.0, 1.0, 2)


def _stages(gen, wf):
    """encoder with its logits, and what the decoder takes beside content and f0 (test_gpu_pitch_path.py's composition)"""
    from tinyvc_amd.module import utils
    eng = gen.engine()
    w = utils.autopad_waveform(wf.to(DEV))
    ssl, _f0, logits = eng.encoder(utils.spectrogram(w), want_logits=True)
    return eng, ssl, logits, utils.estimate_energy(w)


def test_convert_equals_the_stage_composition_with_the_same_state_afterwards(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, logits, energy = _stages(gen, wf)
    blobs, ns = prepare_references(targets)
    start = np.full((B2, 512), -40.0, F)      # a state that knows where the voice was: far from where these logits would start on their own
    start[0, 90], start[1, 400] = 0, 0
    c = PitchCarry(B2, H2, device=DEV)
    c.scores.copy_(_dev(start))
    where = c.scores.data_ptr()
    out = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=SETTINGS2, carry=c)
    state = _dev(start)
    f0, _path, _sc, f0s = eng.pitch_path(logits, SETTINGS2, pitch_shift=SHIFTS2, want_shifted=True, prior=state, carry_out=state, carry_frame=H2)
    want = eng.decoder(eng.knn_match_multi(ssl, blobs, ns), f0s, energy, angle)
    assert torch.equal(out, want), "convert(carry=) != encoder -> pitch_path(prior, carry_out) -> match -> decoder"
    assert torch.equal(c.scores, state) and c.scores.data_ptr() == where and not torch.equal(state, _dev(start)), "the state afterwards"
    uncarried = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=SETTINGS2)
    assert not torch.equal(out, uncarried), "the prior changed nothing on this case: the comparison shows nothing"
    # a fresh carry is the uncarried call's wave, bit for bit (a prior of zeros), and a row equals its own call
    fresh = PitchCarry(B2, H2, device=DEV)
    assert torch.equal(gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=SETTINGS2, carry=fresh), uncarried)
    for b in range(B2):
        one = PitchCarry(1, H2, device=DEV)
        one.scores.copy_(_dev(start[b:b + 1]))
        y = gen.convert(wf[b:b + 1].to(DEV), targets[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), f0_estimation=SETTINGS2, carry=one)
        assert torch.equal(out[b:b + 1], y) and torch.equal(one.scores, c.scores[b:b + 1]), f"row {b} != its own call"


# ---- 6. streams ------------------------------------------------------------------------------------------------------------------------------
def test_streams(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk, shifts = 3, 6, [0.0, 3.0, -2.0]
    tg = [targets[0], targets[1], targets[0]]
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)

    def make(use_graph, f0_carry):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=shifts, device=torch.device(DEV), use_graph=use_graph, f0_estimation="viterbi",
                                f0_carry=f0_carry)
        st.init_buffer()
        return st

    graph, eager, plain = make(True, True), make(False, True), make(False, False)
    assert eager.input_size == 28 * 480 and eager.pitch_carry.params() == (4,) and plain.pitch_carry is None
    assert [name for name, _s, _t in eager._stages()] == ["carry"] and plain._stages() == []
    eng = gen.engine()
    window = torch.zeros(S, eager.input_size, device=DEV)      # the test's own rolling window, state and tail
    own = PitchCarry(S, 4, device=DEV)
    sola = torch.zeros(S, eager.crossfade_size, device=DEV)
    sola_plain = torch.zeros(S, eager.crossfade_size, device=DEV)

    def tail(y, buf):
        return eng.sola(y, buf, eager.fade_in_window, 1920, False, want_shift=True, crossfade=eager.crossfade_size, search=eager.sola_search_size,
                        delay=eager.last_dilay_size)[0]

    captured = None
    for i in range(nblk):
        angle = synth.synth_angle(S, 28, 850 + i).to(DEV)
        if i == 4:      # between replays: stream 1 starts afresh, in place
            before = own.scores.clone()
            for c in (graph.pitch_carry, eager.pitch_carry, own):
                c.reset([1])
        a, b, p = (st.audio_callback(blocks[:, i], noise_angle=angle).clone() for st in (graph, eager, plain))
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(graph.pitch_carry.scores, eager.pitch_carry.scores), f"block {i + 1}: the graph's state != eager's"
        window = torch.cat([window[:, 1920:], blocks[:, i]], dim=1).contiguous()
        assert torch.equal(window, eager.input_wav)
        if i == 4:      # what the block would have been without the reset: streams 0 and 2 are the same, stream 1 is not
            twin = PitchCarry(S, 4, device=DEV)
            twin.scores.copy_(before)
            y_twin = gen.convert(window, tg, shifts, noise_angle=angle, f0_estimation="viterbi", carry=twin)
        y = gen.convert(window, tg, shifts, noise_angle=angle, f0_estimation="viterbi", carry=own)
        assert torch.equal(b, tail(y, sola)), f"block {i + 1} != convert(window, carry=) through the tail"
        assert torch.equal(own.scores, eager.pitch_carry.scores), f"block {i + 1}: the stream's state != the loop's"
        assert float(own.scores.max(dim=1).values.abs().max()) == 0.0
        if i == 4:
            assert torch.equal(y[[0, 2]], y_twin[[0, 2]]) and torch.equal(own.scores[[0, 2]], twin.scores[[0, 2]]), "the reset of stream 1 touched another"
            assert not torch.equal(own.scores[1], twin.scores[1]), "the reset of stream 1 changed nothing"
            assert graph._graph[1][True][0] is captured, "a reset must keep the graph"
        if i == 3:
            captured = graph._graph[1][True][0]      # captured at block 3
        # f0_carry=False is the stream as it was: the uncarried convert of its window
        assert torch.equal(p, tail(gen.convert(window, tg, shifts, noise_angle=angle, f0_estimation="viterbi"), sola_plain)), f"block {i + 1}: f0_carry=False"
    assert not torch.equal(a, p), "the carry changed nothing in six blocks: the comparison shows nothing"
    key = graph._graph_key()
    graph.pitch_carry.hop_frames = 3
    assert graph._graph_key() != key, "hop_frames is baked into the launch: another value must be another key"
    graph.pitch_carry.hop_frames = 4
    assert graph._graph_key() == key
    other = PitchCarry(S, 4, device=DEV)
    graph.pitch_carry = other
    assert graph._graph_key() != key, "another state tensor must be another key"


# ---- 7. the point ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0.25, 0.5, 0.75])
def test_the_carried_window_stays_on_the_ridge_the_uncarried_one_leaves(gen, margin):
    eng, s, T, h = gen.engine(), PitchPath(), 12, 4
    x = C.planted_octave(margin)
    state = torch.zeros(1, 512, device=DEV)
    for n in range(3):
        win = _dev(x[None, :, n * h:n * h + T])
        _f0, path, _sc = eng.pitch_path(win, s, prior=state, carry_out=state, carry_frame=h)
    assert (path == 200).all(), "the carried third window left class 200"
    _f0, alone, _sc = eng.pitch_path(win, s)
    assert (alone == 248).all(), "the uncarried third window is not on the octave: the case shows nothing"
