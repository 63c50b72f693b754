"""The pitch path on the device (tvc_pitch_path_f32, tvc_convert_path_f32, tvc_convert_ragged_path_f32; Engine.pitch_path,
Generator.convert(f0_estimation='viterbi' / PitchPath), BatchedStreamInfer(f0_estimation=)).

Contract (include/tinyvc_hip.h, restated in tests/helpers_pitch_path.py): classes and the last frame's scores equal the numpy fp32
restatement of the full 512 x 512 definition BIT FOR BIT; f0 equals freq[class] bit for bit at refine 0, and at refine r lies within
(4 (2 r + 1) + 2 r) * 2^-24 * truth of the fp64 expectation on the kernel's own path - four roundings per term plus the denominator's adds -
and is exactly 0 where the path is class 0.  A row of a batch equals its own call, a packed ragged call equals its rows alone, two runs are
identical.  The fused conversion equals the stage composition encoder (logits) -> pitch_path -> match -> decoder bit for bit; protect's
share and the automatic shift are those of the path's f0; any other f0_estimation name is the call without the keyword; a captured stream
graph equals eager and another PitchPath is another graph.  The defaults are guesses: nobody has listened."""
import math

import numpy as np
import pytest
import torch

import helpers_pitch_path as H
from helpers import decode_edge_logits, state_dicts
from tinyvc_amd import synth
from tinyvc_amd.engine import pitch_class_table
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = math.inf
SHAPES = [(1, 1), (1, 2), (3, 3), (2, 28), (1, 64), (2, 257), (1, 1024)]
# input kind -> the settings it is decoded under (step, band, jump, voicing, refine)
KINDS = {
    "gaussian": H.DEFAULT,
    "quantised": H.Settings(0.25, 3, 0.75, 0.5, 0),      # jump == band * step, every sum exact, equal candidates everywhere
    "flip": H.DEFAULT._replace(refine=0),
    "dropout": H.DEFAULT._replace(refine=1),
    "special": H.Settings(0.5, 12, INF, 3.0, 4),         # NaN / +-inf columns; jump = +inf
    "edge": H.Settings(0.3, 5, 1.7, INF, 1),             # the per-frame decode's constructed columns; voicing = +inf
}


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


def _logits(kind, B, T):
    """[B, 512, T] fp32, a function of the arguments alone"""
    if kind == "edge":
        return decode_edge_logits(B, T)[0].numpy()
    rows = []
    for b in range(B):
        seed = 1000 * T + 10 * b + 1
        if kind == "gaussian":
            rows.append(H.gaussian(T, seed))
        elif kind == "quantised":
            rows.append(H.quantised(T, seed))
        elif kind == "flip":
            rows.append(H.planted_flip(T, 150 + 40 * b, T // 2, 6.0, seed))
        elif kind == "dropout":
            rows.append(H.planted_dropout(T, 200 + 30 * b, T // 2, 4.0, seed))
        else:
            rows.append(H.special_columns(T, seed))
    return np.stack(rows)


def _path(s):
    return PitchPath(*s)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the stage call against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_bits(gen, shape, kind):
    B, T = shape
    s, freq = KINDS[kind], pitch_class_table().numpy()
    x = _logits(kind, B, T)
    f0, path, scores = (t.cpu().numpy() for t in gen.engine().pitch_path(torch.from_numpy(x).to(DEV), _path(s)))
    assert f0.shape == (B, 1, T) and path.shape == (B, 1, T) and scores.shape == (B, 512)
    for b in range(B):
        want_path, _bp, want_scores = H.viterbi_full(x[b], s)
        assert np.array_equal(path[b, 0], want_path), f"{kind} {shape} row {b}: classes differ at frames {np.nonzero(path[b, 0] != want_path)[0][:8]}"
        assert np.array_equal(_bits(scores[b]), _bits(want_scores)), f"{kind} {shape} row {b}: the last frame's scores differ"
        got = f0[b, 0]
        assert (got[want_path == 0] == 0).all() and (got[want_path != 0] > 20).all()
        if s.refine == 0:
            assert np.array_equal(_bits(got), _bits(np.where(want_path == 0, np.float32(0), freq[want_path])))
        else:
            truth = H.frequency64(x[b], want_path, s.refine, freq)
            err = np.abs(got.astype(np.float64) - truth)
            worst = float((err / np.where(truth > 0, truth, 1.0)).max())
            print(f"[pitch_path] {kind} {shape} row {b}: worst f0 error {worst / 2.0 ** -24:.2f} x 2^-24 of truth (bound {H.f0_bound(s.refine) / 2.0 ** -24:.0f})")
            assert (err <= H.f0_bound(s.refine) * truth).all()
    if kind == "flip" and T >= 3:      # (a single frame has nothing to stay on)
        assert all((path[b, 0] == 150 + 40 * b).all() for b in range(B)), "the planted octave flip left the ridge"
        top4 = gen.engine().pitch_decode(torch.from_numpy(x).to(DEV)).cpu().numpy()      # the per-frame decode does leave it on that frame
        assert all(top4[b, 0, T // 2] > 1.2 * freq[150 + 40 * b] for b in range(B))
    if kind == "dropout" and T >= 3:      # inside a voiced run: frames on both sides
        assert all((path[b, 0] == 200 + 30 * b).all() for b in range(B)), "the planted drop-out was not bridged"


def test_zero_costs_are_the_per_frame_argmax(gen):
    x = np.stack([H.gaussian(64, 5), H.quantised(64, 6)])
    _f0, path, _sc = gen.engine().pitch_path(torch.from_numpy(x).to(DEV), PitchPath(0.0, 12, 0.0, 0.0, 0))
    assert np.array_equal(path[:, 0].cpu().numpy(), np.argmax(x, axis=1))


def test_shifted_output_is_shift_frequency_of_f0(gen):
    eng = gen.engine()
    x = torch.from_numpy(_logits("gaussian", 3, 28)).to(DEV)
    f0, _p, _s, shifted = eng.pitch_path(x, PitchPath(), pitch_shift=[2.0, -3.5, 0.0], want_shifted=True)
    for b, sh in enumerate([2.0, -3.5, 0.0]):
        assert torch.equal(shifted[b], eng.shift_frequency(f0[b:b + 1].contiguous(), sh)[0])


# ---- 2. independence -------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_runs_repeat(gen):
    eng, s = gen.engine(), PitchPath()
    x = torch.from_numpy(np.concatenate([_logits("gaussian", 2, 28), _logits("special", 1, 28), _logits("quantised", 1, 28)])).to(DEV)
    whole = eng.pitch_path(x, s)
    again = eng.pitch_path(x, s)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "two runs differ"
    for b in range(x.shape[0]):
        one = eng.pitch_path(x[b:b + 1].contiguous(), s)
        assert all(torch.equal(w[b:b + 1], o) for w, o in zip(whole, one)), f"row {b} != its own call"


def test_packed_ragged_rows_equal_the_rows_alone(gen):
    eng, s = gen.engine(), PitchPath(refine=1)
    frames = [3, 28, 5]
    rows = [torch.from_numpy(H.gaussian(f, 40 + f)).to(DEV) for f in frames]
    packed = torch.cat(rows, dim=1).contiguous()      # [512, 36]
    start = [0, 3, 31, 36]
    f0, path, scores = eng.pitch_path(packed, s, row_start=start)
    for b, r in enumerate(rows):
        f1, p1, s1 = eng.pitch_path(r[None].contiguous(), s)
        assert torch.equal(f0[0, 0, start[b]:start[b + 1]], f1[0, 0]) and torch.equal(path[0, 0, start[b]:start[b + 1]], p1[0, 0])
        assert torch.equal(scores[b], s1[0]), f"row {b} of the packed call != the row alone"
    # columns outside every row are not written; an empty row writes nothing
    f0g, pathg, _sg = eng.pitch_path(packed, s, row_start=[2, 2, 30])
    assert not f0g[0, 0, :2].any() and not f0g[0, 0, 30:].any() and not pathg[0, 0, 30:].any()


def test_refusals(gen):
    from tinyvc_amd._lib import PitchPathSettings, TinyVCError
    import ctypes
    eng = gen.engine()
    x = torch.zeros(1, 512, 8, device=DEV)
    with pytest.raises(ValueError):
        eng.pitch_path(torch.zeros(1, 511, 8, device=DEV), PitchPath())
    with pytest.raises(ValueError):
        eng.pitch_path(x, PitchPath(), row_start=[0, 9])
    # the library's own host checks, before any device work: settings the Python class would never pass on
    out = torch.full((8,), 7.0, device=DEV)
    I64 = ctypes.c_int64 * 1
    for bad in ((0.5, 12, 5.9, 3.0, 2), (0.5, 33, 99.0, 3.0, 2), (0.5, 12, 12.0, 3.0, 5), (float("nan"), 12, 12.0, 3.0, 2), (0.5, 12, float("nan"), 3.0, 2),
                (0.5, 12, 12.0, float("nan"), 2), (0.5, 12, 12.0, -1.0, 2)):
        rc = eng.lib.tvc_pitch_path_f32(eng.ctx, eng._stream(), x.data_ptr(), I64(0), I64(8), 1, 8, ctypes.byref(PitchPathSettings(*bad)), 0.0, None,
                                        out.data_ptr(), None, None, None, None, 0)
        assert rc != 0 and b"path" in eng.lib.tvc_last_error(eng.ctx), bad
    assert (out == 7.0).all()
    with pytest.raises(ValueError, match="f0_estimation"):
        gen.convert(torch.zeros(1, 4800, device=DEV), synth.synth_index(300, seed=21).to(DEV), 0.0, f0_estimation=PitchPath(jump=1.0))
    assert TinyVCError is not None


# ---- 3. the fused conversion ------------------------------------------------------------------------------------------------------------
B2, T2 = 2, 28
SHIFTS2 = [2.0, -3.0]
SETTINGS2 = PitchPath(0.5, 12, 12.0, 1.0, 2)


def _stages(gen, wf):
    """encoder with its logits, and what the decoder takes beside content and f0"""
    from tinyvc_amd.module import utils
    eng = gen.engine()
    w = utils.autopad_waveform(wf.to(DEV))
    ssl, f0_top4, logits = eng.encoder(utils.spectrogram(w), want_logits=True)
    return eng, ssl, logits, utils.estimate_energy(w), f0_top4


def _prepared(tg):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    return prepare_references(tg)


def test_convert_equals_the_stage_composition(gen, targets):
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, logits, energy, f0_top4 = _stages(gen, wf)
    blobs, ns = _prepared(targets)
    f0, path, _sc, f0s = eng.pitch_path(logits, SETTINGS2, pitch_shift=SHIFTS2, want_shifted=True)
    assert not torch.equal(f0, f0_top4), "the path's f0 is the per-frame decode's on this case: the comparison shows nothing"
    out = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=SETTINGS2)
    want = eng.decoder(eng.knn_match_multi(ssl, blobs, ns), f0s, energy, angle)
    assert torch.equal(out, want), "convert(f0_estimation=PitchPath) != encoder -> pitch_path -> match -> decoder"
    plain = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle)
    assert not torch.equal(out, plain)
    # every other name is the call without the keyword
    for name in ("default", "harvest"):
        assert torch.equal(gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=name), plain)
    # 'viterbi' is PitchPath() with the defaults; a row equals its own call; one shared index takes the same entry
    vit = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation="viterbi")
    assert torch.equal(vit, gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, f0_estimation=PitchPath()))
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), targets[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), f0_estimation=SETTINGS2)
        assert torch.equal(out[b:b + 1], one), f"row {b} != its own call"
    shared = gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, f0_estimation=SETTINGS2)
    f0s1 = eng.pitch_path(logits, SETTINGS2, pitch_shift=1.0, want_shifted=True)[3]
    assert torch.equal(shared, eng.decoder(eng.knn_match_multi(ssl, [blobs[1]] * B2, [ns[1]] * B2), f0s1, energy, angle))


def test_convert_protect_and_auto_pitch_read_the_path(gen, targets):
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, logits, energy, _f0 = _stages(gen, wf)
    blobs, ns = _prepared(targets)
    alpha, protect = torch.tensor([0.3, 0.0], device=DEV), torch.tensor([0.5, 1.0], device=DEV)
    f0, _p, _sc, f0s = eng.pitch_path(logits, SETTINGS2, pitch_shift=SHIFTS2, want_shifted=True)
    assert (f0 > 0).any() and not (f0 > 0).all(), "the case holds no unvoiced frame: protect shows nothing"
    # protect: the share is frame_share of the path's f0
    out = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, alpha=alpha, protect=protect, f0_estimation=SETTINGS2)
    matched = eng.knn_match_protect(ssl, f0, blobs, ns, alpha, protect)
    assert torch.equal(out, eng.decoder(matched, f0s, energy, angle)), "protect does not read the path's f0"
    # auto pitch: the shifts are pitch_match of the path's f0
    reg = torch.tensor([180.0, 240.0], device=DEV)
    out, sh = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, f0_estimation=SETTINGS2)
    _med, _voiced, want_sh, want_f0s = eng.pitch_match(f0, target_f0=reg, pitch_shift=SHIFTS2, want_shifted=True)
    assert torch.equal(sh, want_sh), "the automatic shifts are not pitch_match of the path's f0"
    assert torch.equal(out, eng.decoder(eng.knn_match_multi(ssl, blobs, ns), want_f0s, energy, angle))
    # with loudness and limit behind it the call runs and stays finite
    y = gen.convert(wf.to(DEV), targets, SHIFTS2, noise_angle=angle, alpha=alpha, protect=protect, loudness=0.5, limit=-1.0, f0_estimation="viterbi")
    assert torch.isfinite(y).all() and float(y.abs().max()) <= 10 ** (-1 / 20) * (1 + 1e-6)


def test_convert_ragged(gen, targets):
    frames = [7, 33, 20]
    lens = [480 * f - (11 if i % 2 else 0) for i, f in enumerate(frames)]
    B, Tmax = len(frames), max(frames)
    wf = torch.zeros(B, 480 * Tmax)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=600 + b)[0]
    tg = [targets[b % 2] for b in range(B)]
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    out = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, f0_estimation=SETTINGS2)
    blobs, ns = _prepared(tg)
    for b, f in enumerate(frames):
        eng, ssl, logits, energy, _f0 = _stages(gen, wf[b:b + 1, :lens[b]])
        f0s = eng.pitch_path(logits, SETTINGS2, pitch_shift=-2.0, want_shifted=True)[3]
        want = eng.decoder(eng.knn_match_multi(ssl, blobs[b:b + 1], ns[b:b + 1]), f0s, energy, angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b:b + 1, :480 * f], want), f"row {b} ({f} frames) != its own stage composition"
        assert not out[b, 480 * f:].any()


# ---- 4. streams -------------------------------------------------------------------------------------------------------------------------
def test_streams_graph_equals_eager_and_settings_are_part_of_the_key(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk = 2, 5
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)
    sts = {}
    for use_graph in (True, False):
        st = BatchedStreamInfer(gen, n_streams=S, target=targets, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840,
                                use_graph=use_graph, f0_estimation="viterbi")
        st.init_buffer()
        sts[use_graph] = st

    def block(i):
        angle = synth.synth_angle(S, sts[True].input_size // 480, 850 + i).to(DEV)
        a, b = (sts[g].audio_callback(blocks[:, i], noise_angle=angle).clone() for g in (True, False))
        return a, b, angle

    eng, eager = gen.engine(), sts[False]
    for i in range(3):
        sola_before = eager.sola_buffer.clone()
        a, b, angle = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        # each block is convert of its window, through the stream's own tail
        y = gen.convert(eager.input_wav, targets, [0.0, 3.0], noise_angle=angle, f0_estimation="viterbi")
        want = eng.sola(y, sola_before, eager.fade_in_window, 1920, False, want_shift=True, crossfade=eager.crossfade_size, search=eager.sola_search_size,
                        delay=eager.last_dilay_size)[0]
        assert torch.equal(b, want), f"block {i + 1} != convert of its window"
    captured = sts[True]._graph[1][True][0]      # captured at block 3
    other = PitchPath(0.25, 8, 4.0, 0.5, 0)
    for g in (True, False):
        sts[g].f0_estimation = other
    a, b, _angle = block(3)
    assert torch.equal(a, b), "block 4: the replay is stale - it did not follow the new settings"
    assert sts[True]._graph[1][True][0] is not captured, "another PitchPath must be another graph"
    fresh = sts[True]._graph[1][True][0]
    a, b, _angle = block(4)
    assert torch.equal(a, b) and sts[True]._graph[1][True][0] is fresh
    # and the path does something in a stream: the same settings' window conversion differs from the per-frame decode's
    assert not torch.equal(y, gen.convert(sts[False].input_wav, targets, [0.0, 3.0], noise_angle=angle))
