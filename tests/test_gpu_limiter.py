"""The look-ahead peak limiter on the GPU (tvc_limit_f32, tvc_stream_limit_f32; the definition is in include/tinyvc_hip.h) against its numpy
fp32 restatement (helpers_limiter).

Bounds.  Peaks, max, min and compares are exact; every other step of the definition is one correctly rounded fp32 operation, which numpy
float32 performs identically.  So gains and samples are held BIT FOR BIT, everywhere.  The one exception is reduction_db: ocml's log10f is
good to about 2 ulp (2e-5 dB at -120 dB), so it is held within 1e-3 dB of the fp64 20 log10 of the kernel's own fp32 gain - a bound that
catches only a wrong formula."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import helpers_limiter as H
from helpers import state_dicts
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CEILINGS = [0.5, 10.0 ** (-1.0 / 20.0), math.inf]


def _engine():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _bits(x):
    x = torch.as_tensor(x).cpu().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    """bit for bit (torch.equal would call -0.0 and 0.0 equal and a NaN unequal to itself)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype).to(DEV).contiguous()


def _settings(sub=4, release=3, drive_db=0.0):
    return types.SimpleNamespace(sub_frame=sub, release=release, drive_db=drive_db)


@pytest.fixture(scope="module")
def consts():
    """(T, C): the offline tile and the stream chunk, in sub-frames"""
    from tinyvc_amd.engine import limiter_geometry
    return limiter_geometry(4 * 8, 4, 1)[2], limiter_geometry(4 * 8, 4, 1, stream_block=True)[2]


def _rows(T, sub, R, seed=5):
    """B = 3 rows of 2T + 3 sub-frames: noise at 0.3 with bursts of 4.0 in the row's first and last sub-frame, the last sub-frame of a tile,
    the first of the next, and R + 1 and R + 2 sub-frames in front of a tile edge"""
    K = 2 * T + 3
    rng = np.random.default_rng(seed + R + sub)
    where = [0, K - 1, T - 1, T, T - (R + 1), T - (R + 2), 2 * T - (R + 1), 2 * T - (R + 2), 2 * T - 1, 2 * T]
    return np.stack([H.bursty(rng, K * sub, sub, bursts=where) for _ in range(3)])


# ---- 1. offline against the restatement -------------------------------------------------------------------------------------------------------
def _offline_cases(T):
    return [(4, 1, 0.0), (4, 3, 0.0), (4, T + 2, 0.0), (24, 3, 6.0)]


@pytest.mark.parametrize("case", range(4), ids=["R1", "R3", "R_tile_plus_2", "sub24_drive6"])
def test_offline_equals_the_restatement_bit_for_bit(consts, case):
    T = consts[0]
    sub, R, drive_db = _offline_cases(T)[case]
    y = _rows(T, sub, R)
    out, gains = _engine().limit(_dev(y), _dev(CEILINGS), settings=_settings(sub, R, drive_db), want_gains=True)
    out, gains = out.cpu().numpy(), gains.cpu().numpy()
    assert gains.shape == (3, y.shape[1] // sub + 1)
    for b in range(3):
        want, wg = H.limit(y[b], CEILINGS[b], sub, R, drive_db)
        bad = np.flatnonzero(H.bits(gains[b]) != H.bits(wg))
        assert bad.size == 0, f"row {b}: {bad.size} gains differ, first at edge {bad[:1]}: {gains[b][bad[:1]]} against {wg[bad[:1]]}"
        bad = np.flatnonzero(H.bits(out[b]) != H.bits(want))
        assert bad.size == 0, f"row {b}: {bad.size} samples differ, first at {bad[:1]}"
        c = H.ceiling_of(CEILINGS[b])
        assert bool((np.abs(out[b]) <= c).all()), f"row {b}: a sample above its ceiling"
        if b < 2:
            assert gains[b].min() < 0.25 and float(np.abs(out[b]).max()) >= 0.999 * float(c), "the limiter hardly worked: the case shows nothing"
    if drive_db == 0.0:
        assert np.array_equal(H.bits(out[2]), H.bits(y[2])) and bool((gains[2] == 1.0).all()), "a ceiling of inf changed a bit"


# ---- 2. ragged --------------------------------------------------------------------------------------------------------------------------------
def test_ragged_rows_equal_their_own_calls_and_the_call_is_capturable(consts):
    T, sub, R = consts[0], 4, 3
    eng = _engine()
    y3 = _rows(T, sub, R, seed=9)
    L = y3.shape[1]
    lens = [0, sub, L - sub, L, L - 2 * sub - 3]
    y = np.stack([y3[0], y3[1], y3[2], y3[0], y3[1]])
    ceil = _dev([0.5, 0.4, 0.6, 0.7, 0.3])
    Y = _dev(y)
    out, gains = eng.limit(Y, ceil, lengths=lens, settings=_settings(sub, R), want_gains=True)
    for b, n in enumerate(lens):
        n = n // sub * sub
        assert _same(out[b, n:], Y[b, n:]), f"row {b}: the samples behind its length are not y's"
        assert bool((gains[b, n // sub + 1:] == 1.0).all()), f"row {b}: gains behind its length"
        want, wg = H.limit(y[b], ceil[b].item(), sub, R, length=lens[b])
        assert np.array_equal(H.bits(out[b].cpu().numpy()), H.bits(want)) and np.array_equal(H.bits(gains[b].cpu().numpy()), H.bits(wg)), f"row {b}"
        if n:
            alone, ga = eng.limit(Y[b:b + 1, :n].contiguous(), ceil[b:b + 1].contiguous(), settings=_settings(sub, R), want_gains=True)
            assert _same(alone[0], out[b, :n]) and _same(ga[0], gains[b, :n // sub + 1]), f"row {b}: not the call on the row alone"
    buf = Y.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # a copy from the host or a synchronisation would fail the capture
        cap = eng.limit(buf, ceil, lengths=lens, settings=_settings(sub, R))
    buf.copy_(Y.flip(0))
    g.replay()
    buf.copy_(Y)
    g.replay()
    torch.cuda.synchronize()
    assert _same(cap, out), "the replay is not the eager call"


# ---- 3. a stream is the offline result, delayed -------------------------------------------------------------------------------------------------
def _stage(S, block, sub=4, release=3, ceiling=None, drive_db=0.0):
    from tinyvc_amd.module.infer import StreamLimiter
    st = StreamLimiter(S, block, ceiling_db=0.0, sub_frame=sub, release_size=release * sub, drive_db=drive_db, device=DEV)
    if ceiling is not None:
        st.ceiling.copy_(_dev(ceiling))
    return st


def _state(stage):
    return {k: getattr(stage, k).clone() for k in ("tail", "peak", "gain")}


def _run_stream(y, per_block, sub, R, ceilings):
    """y [S, n] cut into blocks of per_block sub-frames (the rest is dropped) -> (concatenated output, concatenated inner gains, state)"""
    eng = _engine()
    S, block = y.shape[0], per_block * sub
    stage = _stage(S, block, sub, R, ceilings)
    outs, gs = [], []
    for i in range(y.shape[1] // block):
        o, g = eng.stream_limit(_dev(y[:, i * block:(i + 1) * block]), stage, want_gains=True)
        outs.append(o)
        gs.append(g[:, 1:] if i else g)
        red = stage.reduction_db.cpu().double()
        want = 20.0 * torch.log10(g.cpu().double().min(dim=1).values)
        assert bool((((red - want).abs() <= 1e-3) | (red == want)).all()), f"reduction_db {red.tolist()} against {want.tolist()}"
    return torch.cat(outs, dim=1), torch.cat(gs, dim=1), _state(stage)


def test_a_stream_is_the_offline_result_delayed_however_it_is_cut(consts):
    T, C = consts
    sub, R = 4, 3
    y = _rows(T, sub, R)
    offline, og = _engine().limit(_dev(y), _dev(CEILINGS), settings=_settings(sub, R), want_gains=True)
    n = (C + 1) * sub * (y.shape[1] // ((C + 1) * sub))      # a length all three cuts reach: whole blocks of C + 1 sub-frames (an even count)
    assert n >= (C + 1) * sub and n % (2 * sub) == 0
    states = []
    for per in (1, 2, C + 1):
        out, gains, state = _run_stream(y[:, :n], per, sub, R, CEILINGS)
        want = torch.cat([torch.zeros(3, sub, device=DEV), offline[:, :n - sub]], dim=1)
        assert _same(out, want), f"{per} sub-frames per block: not the offline result behind {sub} zeros"
        assert _same(gains[:, 1:], og[:, :n // sub]), f"{per} sub-frames per block: the gains"      # (edge 0 of a stream is the start's 1.0)
        states.append(state)
    assert all(_same(states[0][k], s[k]) for s in states[1:] for k in s), "the final state depends on the cut"
    alone, _, st1 = _run_stream(y[1:2, :n], 2, sub, R, CEILINGS[1:2])
    three, _, st3 = _run_stream(y[:, :n], 2, sub, R, CEILINGS)
    assert _same(alone[0], three[1]) and all(_same(st1[k][0], st3[k][1]) for k in st1), "S = 1 is not the stream's row inside S = 3"


# ---- 4. live parameters under one graph ---------------------------------------------------------------------------------------------------------
def test_one_captured_launch_follows_ceiling_and_reset():
    eng = _engine()
    sub, R, S, per = 4, 3, 3, 5
    rng = np.random.default_rng(3)
    blocks = [np.stack([H.bursty(rng, per * sub, sub, bursts=[i % per]) for _ in range(S)]) for i in range(6)]
    graph, eager = _stage(S, per * sub, sub, R, [0.5, 0.4, 0.6]), _stage(S, per * sub, sub, R, [0.5, 0.4, 0.6])
    buf = _dev(blocks[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):      # capture runs nothing: the state is still the start's
        cap = eng.stream_limit(buf, graph)
    for i, blk in enumerate(blocks):
        for st in (graph, eager):
            if i == 2:
                st.ceiling.fill_(0.25)
            if i == 3:
                st.set_ceiling_db([-6.0, math.inf, -20.0])
            if i == 4:
                st.reset([1])
        buf.copy_(_dev(blk))
        g.replay()
        want = eng.stream_limit(_dev(blk), eager)
        assert _same(cap, want), f"block {i}: the replay is not the eager call from the same state"
        assert all(_same(getattr(graph, k), getattr(eager, k)) for k in ("tail", "peak", "gain", "reduction_db")), f"block {i}: the state"
    assert eager.ceiling.tolist() == [F(10.0 ** (-6.0 / 20.0)), math.inf, F(10.0 ** (-20.0 / 20.0))]


# ---- 5. non-finite input ------------------------------------------------------------------------------------------------------------------------
def test_nan_moves_no_gain_and_inf_closes_its_edges():
    eng = _engine()
    sub, R, per = 4, 3, 8
    rng = np.random.default_rng(8)
    y = (rng.standard_normal((1, per * sub)) * 0.3).astype(F)
    clean = y.copy()
    y[0, 2 * sub + 1] = np.nan
    stage, ref = _stage(1, per * sub, sub, R, [0.5]), _stage(1, per * sub, sub, R, [0.5])
    o, g = eng.stream_limit(_dev(y), stage, want_gains=True)
    oc, gc = eng.stream_limit(_dev(clean), ref, want_gains=True)
    o, oc = o.cpu().numpy()[0], oc.cpu().numpy()[0]
    assert _same(g, gc), "a NaN sample moved a gain"
    at = 3 * sub + 1      # (one sub-frame late)
    assert np.isnan(o[at]) and np.array_equal(H.bits(np.delete(o, at)), H.bits(np.delete(oc, at))) and bool(np.isfinite(np.delete(o, at)).all())
    z = clean.copy()
    z[0, 4 * sub + 2] = np.inf
    closed = _stage(1, per * sub, sub, R, [0.5])
    o, g = eng.stream_limit(_dev(z), closed, want_gains=True)
    o, g = o.cpu().numpy()[0], g.cpu().numpy()[0]
    assert g[5] == 0.0 and g[6] == 0.0, f"the edges around an infinite sample: {g[5:7]}"      # (g[0] is the carried gain: edge k of the block is g[k + 1])
    at = 5 * sub + 2
    assert np.isnan(o[at]) and bool(np.isfinite(np.delete(o, at)).all())
    want, wg = H.Stream(sub, R).block(z[0], 0.5)
    assert H.same_bits(o, want) and H.same_bits(g, wg)
    # ... and offline; the state behind a block whose last sub-frame is clean is finite
    off, og = eng.limit(_dev(z), _dev([0.5]), settings=_settings(sub, R), want_gains=True)
    want, wg = H.limit(z[0], 0.5, sub, R)
    assert H.same_bits(off.cpu().numpy()[0], want) and H.same_bits(og.cpu().numpy()[0], wg)
    for st in (stage, closed):
        for k in ("tail", "peak", "gain"):
            assert bool(torch.isfinite(getattr(st, k)).all()), f"{k} after the block"


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    eng = _engine()
    lib, ctx = eng.lib, eng.ctx
    y, out = _dev(np.zeros((2, 64), F)), _dev(np.zeros((2, 64), F))
    ceil, tail, peak, gain = _dev([0.5, 0.5]), _dev(np.zeros((2, 4), F)), _dev([0.0, 0.0]), _dev([1.0, 1.0])
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def offline(y_=y, out_=out, B=2, L=64, ceil_=ceil, sub=4, R=3, drive=0.0):
        return lib.tvc_limit_f32(ctx, None, p(y_), p(out_), B, L, None, p(ceil_), sub, R, drive, None)

    def stream(y_=y, out_=out, S=2, block=64, sub=4, R=3, drive=0.0, ceil_=ceil, tail_=tail, peak_=peak, gain_=gain):
        return lib.tvc_stream_limit_f32(ctx, None, p(y_), p(out_), S, block, sub, R, drive, p(ceil_), p(tail_), p(peak_), p(gain_), None, None)

    before = (_bits(out).clone(), _bits(tail).clone())
    for call, text in ((lambda: offline(out_=y), "out overlaps y"), (lambda: offline(out_=y[1:]), "out overlaps y"), (lambda: stream(out_=y), "out overlaps y"),
                       (lambda: offline(y_=None), "NULL"), (lambda: offline(ceil_=None), "NULL"), (lambda: offline(B=0), "B <= 0"),
                       (lambda: stream(tail_=None), "NULL"), (lambda: stream(gain_=None), "NULL"), (lambda: stream(S=0), "S <= 0"),
                       (lambda: offline(drive=math.nan), "drive_db"), (lambda: offline(drive=math.inf), "drive_db"), (lambda: stream(drive=2000.0), "drive_db"),
                       (lambda: stream(drive=-2000.0), "drive_db"),
                       (lambda: stream(block=66), "not a whole number"), (lambda: stream(block=0), "block = 0"),
                       (lambda: offline(L=66), "not a whole number"), (lambda: offline(sub=6), "multiple of 4"), (lambda: offline(R=0), "release = 0"),
                       (lambda: stream(R=4097), "release = 4097")):
        assert call() != 0
        assert text in lib.tvc_last_error(ctx).decode(), f"{lib.tvc_last_error(ctx).decode()!r} does not say {text!r}"
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before[0]) and torch.equal(_bits(tail), before[1]), "a refused call wrote something"
    assert offline() == 0 and stream() == 0
    from tinyvc_amd._lib import TinyVCError
    with pytest.raises(TinyVCError, match="block = 66 is not a whole number"):      # a stage that got past the Python checks: the library's own refusal
        eng.stream_limit(_dev(np.zeros((2, 66), F)), types.SimpleNamespace(n_streams=2, block_size=66, ceiling=ceil, tail=tail, peak=peak, gain=gain,
                                                                           reduction_db=_dev([0.0, 0.0]), sub_frame=4, params=lambda: (2, 66, 4, 3, 0.0)))


# ---- 9. the point of it -------------------------------------------------------------------------------------------------------------------------
def test_behind_the_limiter_the_door_no_longer_wraps():
    from tinyvc_amd.module.infer import StreamDoor, StreamLimiter
    eng = _engine()
    S, block, sub = 2, 480, 24
    rng = np.random.default_rng(4)
    y = np.stack([H.bursty(rng, 6 * block, sub, level=0.3, burst=3.0, bursts=range(3, 120, 7)) for _ in range(S)])
    y[:, 1000] = 1.0      # a sample of exactly 1.0 wraps too
    assert float(np.abs(y).max()) == 3.0
    stage = StreamLimiter(S, block, ceiling_db=-1.0, device=DEV)
    door, bare = StreamDoor(S, 24000, block_size=block, device=DEV), StreamDoor(S, 24000, block_size=block, device=DEV)
    door.prepare(eng), bare.prepare(eng)
    pcm, direct = [], []
    for i in range(6):
        blk = _dev(y[:, i * block:(i + 1) * block])
        pcm.append(door.pull(eng, eng.stream_limit(blk, stage)))
        direct.append(bare.pull(eng, blk))
    pcm, direct = torch.cat(pcm, 1).cpu().numpy().astype(np.int64), torch.cat(direct, 1).cpu().numpy().astype(np.int64)
    late = door.delay_out      # (24 kHz samples: the rates are equal)
    c = float(stage.ceiling[0])
    assert int(np.abs(pcm).max()) <= math.floor(c * 32768), f"max |pcm| = {np.abs(pcm).max()} above floor(c * 32768) = {math.floor(c * 32768)}"
    assert int(np.abs(pcm).max()) >= math.floor(c * 32768) - 1, "the ceiling was never reached: the case shows nothing"
    src = np.concatenate([np.zeros((S, sub + late), F), y], 1)[:, :pcm.shape[1]]
    assert bool((pcm * np.sign(src) >= 0).all()), "a limited sample left with the other sign"
    src = np.concatenate([np.zeros((S, late), F), y], 1)[:, :direct.shape[1]]
    wrapped = int((direct * np.sign(src) < 0).sum())
    assert wrapped > 0 and direct[0, 1000 + late] == -32768, "without the limiter nothing wrapped: the test would pass without the feature"
    print(f"without the limiter {wrapped} samples wrapped; with it max |pcm| = {np.abs(pcm).max()}")


# ---- 7. through the chain ---------------------------------------------------------------------------------------------------------------------
GEOM = dict(block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3840)      # a window of 4320: nine whole frames
S3, SUB = 3, 24


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
def model_side():
    tgt = synth.synth_index(1000, seed=2).to(DEV)
    angles = [synth.synth_angle(S3, 9, 700 + i).to(DEV) for i in range(6)]
    mic = (synth.synth_wave(S3, 6 * 480, seed=21) * 0.9).to(DEV)
    return tgt, angles, mic


def _stream(gen, tgt, use_graph=False, **stages):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=S3, target=tgt, pitch_shift=[0.0, 2.0, -1.5], device=torch.device(DEV), use_graph=use_graph, **stages, **GEOM)
    st.init_buffer()
    return st


@pytest.fixture(scope="module")
def plain_blocks(gen, model_side):
    """the stream without the stage, once: its blocks [n][S3, 480]"""
    tgt, angles, mic = model_side
    st = _stream(gen, tgt)
    return [st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i]).clone() for i in range(5)], st.latency_samples


def test_in_a_stream_the_stage_is_the_last_launch(gen, model_side, plain_blocks):
    from tinyvc_amd.module.infer import StreamLimiter
    tgt, angles, mic = model_side
    plain, latency = plain_blocks
    eng = gen.engine(torch.device(DEV))
    off = _stream(gen, tgt, limiter=StreamLimiter(S3, 480, ceiling_db=math.inf, device=DEV))
    assert off.latency_samples == (latency[0] + SUB, latency[1] + SUB)
    peak = float(torch.cat(plain, 1).abs().max())
    db = 20.0 * math.log10(peak) - 12.0      # a ceiling the stream's own peaks lie 12 dB above
    fin, hand = _stream(gen, tgt, limiter=StreamLimiter(S3, 480, ceiling_db=db, device=DEV)), StreamLimiter(S3, 480, ceiling_db=db, device=DEV)
    got = []
    for i in range(5):
        blk = mic[:, i * 480:(i + 1) * 480]
        got.append(off.audio_callback(blk, noise_angle=angles[i]).clone())
        out = fin.audio_callback(blk, noise_angle=angles[i])
        assert _same(out, eng.stream_limit(plain[i], hand)), f"block {i}: not the stage applied to the plain stream's block"
        assert float(out.abs().max()) <= float(hand.ceiling[0])
    assert float(hand.reduction_db.min()) < -6.0, "the limiter hardly worked"
    want = torch.cat([torch.zeros(S3, SUB, device=DEV), torch.cat(plain, 1)[:, :-SUB]], 1)
    assert _same(torch.cat(got, 1), want), "with a ceiling of inf the stream is not the plain one, one sub-frame late"


def test_in_a_stream_graph_replay_equals_eager(gen, model_side):
    from tinyvc_amd.module.infer import StreamLimiter
    tgt, angles, mic = model_side
    outs = {}
    for use_graph in (False, True):
        stage = StreamLimiter(S3, 480, ceiling_db=-30.0, device=DEV)
        st = _stream(gen, tgt, use_graph, limiter=stage)
        res = []
        for i in range(5):
            if i == 3:
                stage.set_ceiling_db(-40.0, streams=[0, 2])
            res.append(st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i]).clone())
        outs[use_graph] = (torch.stack(res), _state(stage))
        if use_graph:
            assert st._graph is not None and any(k[0] == "limiter" for k in st._graph[0] if isinstance(k, tuple) and k and isinstance(k[0], str))
    assert _same(outs[True][0], outs[False][0]) and all(_same(outs[True][1][k], outs[False][1][k]) for k in outs[True][1])


# ---- 8. Generator.convert ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["equal", "ragged", "loudness", "auto_pitch"])
def test_convert_with_limit_is_the_launch_behind_everything_else(gen, case):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Limiter
    from tinyvc_amd.module.utils import autopad_waveform
    eng = gen.engine(torch.device(DEV))
    wf = (synth.synth_wave(2, 9500, seed=1) * torch.tensor([[1.0], [0.3]])).to(DEV)      # (9500 is padded to 9600)
    tgt = synth.synth_index(256, seed=2).to(DEV)
    angle = synth.synth_angle(2, 20, 3).to(DEV)
    kw = dict(equal={}, ragged=dict(lengths=[9500, 7000]), loudness=dict(loudness=[0.8, 1.0]), auto_pitch=dict(auto_pitch=180.0, return_shift=True))[case]
    plain = gen.convert(wf, tgt, 1.0, noise_angle=angle, **kw)
    wave = plain[0] if case == "auto_pitch" else plain
    db = 20.0 * math.log10(float(wave.abs().max())) - 12.0
    got = gen.convert(wf, tgt, 1.0, noise_angle=angle, limit=[db, db - 6.0], **kw)
    if case == "auto_pitch":
        assert isinstance(got, tuple) and _same(got[1], plain[1])
        got = got[0]
    ceil = _dev([10.0 ** (db / 20.0), 10.0 ** ((db - 6.0) / 20.0)], torch.float64).float()
    lens = [9600, 7200] if case == "ragged" else None
    want = eng.limit(wave, ceil, lengths=lens)
    assert _same(got, want) and not _same(got, wave), case
    assert bool((got[0].abs() <= ceil[0]).all()) and bool((got[1, :7200].abs() <= ceil[1]).all())
    if case == "loudness":      # loudness first, then the limit: the other order gives another wave
        bare = gen.convert(wf, tgt, 1.0, noise_angle=angle)
        other = eng.loudness_match(autopad_waveform(wf), eng.limit(bare, ceil), _dev([0.8, 1.0]))
        assert not _same(got, other)
    if case == "equal":      # the settings ride on a Limiter, the ceilings on a device tensor of linear values used in place
        got = gen.convert(wf, tgt, 1.0, noise_angle=angle, limit=Limiter(ceil, sub_frame=48, release_size=480, drive_db=3.0))
        assert _same(got, eng.limit(wave, ceil, settings=types.SimpleNamespace(sub_frame=48, release=10, drive_db=3.0)))
        with pytest.raises(ValueError, match="does not divide the 480-sample frames"):
            gen.convert(wf, tgt, 1.0, noise_angle=angle, limit=Limiter(db, sub_frame=36, release_size=360))


# ---- 10. the entry scripts --------------------------------------------------------------------------------------------------------------------
def test_infer_py_limit_whole_files_and_chunked(tmp_path):
    import infer
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(300, seed=2), d / "a.pt")
    (d / "inputs").mkdir()
    audio_io.save(str(d / "inputs" / "x.wav"), synth.synth_wave(1, 12000, seed=3) * 0.9, 24000)
    common = ["-i", str(d / "inputs"), "-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "a.pt"), "-p", "1.0", "-d", DEV, "--seed", "3"]
    assert infer.main(common + ["-o", str(d / "plain")]) == 0
    plain = audio_io.load(str(d / "plain" / "x.wav"))[0]
    db = 20.0 * math.log10(float(plain.abs().max())) - 12.0
    c = float(F(10.0 ** (db / 20.0)))
    assert infer.main(common + ["-o", str(d / "whole"), "--limit", repr(db)]) == 0
    whole = audio_io.load(str(d / "whole" / "x.wav"))[0]
    assert whole.shape == plain.shape and float(whole.abs().max()) <= c < float(plain.abs().max())
    chunk = ["--chunked", "-c", "1920"]
    assert infer.main(common + chunk + ["-o", str(d / "cplain")]) == 0
    assert infer.main(common + chunk + ["-o", str(d / "climit"), "--limit", repr(db)]) == 0
    a, b = audio_io.load(str(d / "cplain" / "x.wav"))[0][0].double(), audio_io.load(str(d / "climit" / "x.wav"))[0][0].double()
    assert a.shape == b.shape and float(b.abs().max()) <= c
    # time-aligned: with the same seed the limited stream is the unlimited one under the limiter, one sub-frame late, and that sub-frame
    # is in the trim.  A gain depends on the last R + 1 = 101 sub-frames only, so from 102 sub-frames into the file the offline restatement
    # of the unlimited file IS the limited file, bit for bit, on the stream's sub-frame grid - which starts at one of 24 offsets into the
    # trimmed file.  A trim that is a sample off in either direction matches at none of them.
    a32, b32 = a.float().numpy(), b.float().numpy()
    warm, hits = 102 * 24, []
    for o in range(24):
        n = (len(a32) - o) // 24 * 24
        want = H.limit(a32[o:o + n], c, 24, 100)[0]
        hits.append(bool(np.array_equal(H.bits(want[warm:]), H.bits(b32[o + warm:o + n]))))
    assert sum(hits) == 1, f"the limited file is the limiter of the unlimited one at {sum(hits)} of the 24 grid offsets: the trim is off"
    assert not np.array_equal(a32[warm:], b32[warm:]), "the limiter changed nothing: the case shows nothing"
    # (and the issue's own figure: the normalised cross-correlation of the first block pair at lag 0.  b = g a with g in [g_min, 1] gives
    # at least 2 sqrt(g_min) / (1 + g_min) (Kantorovich): 0.8 at the 12 dB the ceiling lies under the peak)
    assert bool((a * b >= 0).all()) and bool((b.abs() <= a.abs()).all()), "a limited sample with the other sign, or a larger one"
    n = 1920
    rho = float((a[:n] * b[:n]).sum() / (a[:n].pow(2).sum() * b[:n].pow(2).sum()).sqrt())
    print(f"chunked: normalised cross-correlation at lag 0 over the first block pair {rho:.4f}")
    assert rho >= 0.8
