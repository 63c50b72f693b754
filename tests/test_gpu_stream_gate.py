"""The streams' noise gate on the device (tvc_stream_gate_f32; Engine.stream_gate, module.infer.StreamGate, BatchedStreamInfer(gate=...),
infer_streaming.py --gate).

The file carries its own restatement of the definition in tinyvc_hip.h (`_restate`): the serial scan in numpy float32 scalar operations,
everything else - sub-frame powers, thresholds, the per-sample ramp - in fp64.  Inputs are +-0.5 square-wave bursts on a +-1e-4 floor with
burst edges at arbitrary samples, thresholds -40 dB with 6 dB of hysteresis: a sub-frame holding one loud sample has a power of at least
0.25 / 240 (-30 dB), a pure-floor one is at -80 dB, and every test asserts ON ITS OWN INPUTS that each fp64 `d` is at least 3 dB from both
thresholds.  That is a condition, not a tolerance: it makes every open / close decision independent of the fp32 summation order, so
  open, hold   are equal as integers,
  gain         is equal bit for bit (defined as single fp32 adds and clamps),
  level_db     is within 1e-3 dB,
  every sample is within 2^-21 |y| of the fp64 evaluation of y * ramp on those fp32 end-point gains (at most eight fp32 roundings lie
               between y and out, each at most 2^-24 of a multiplier that is at most 1)."""
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

from helpers import state_dicts
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR, HYST = -40.0, 6.0
SAMPLE_BOUND = 2.0 ** -21
LEVEL_BOUND_DB = 1e-3


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


def _bursts(S, length, seed, period=7):
    """[S, length] fp32: a square wave of `period` samples, +-0.5 inside bursts and +-1e-4 outside; burst edges at arbitrary samples.
    Stream 0 is floor only, stream 1 one burst from end to end, the others carry a few bursts with silences long enough to close a gate."""
    rng = np.random.default_rng(seed)
    sign = np.where((np.arange(length) // period) % 2 == 0, 1.0, -1.0)
    x = np.empty((S, length), dtype=np.float32)
    for s in range(S):
        loud = np.zeros(length, dtype=bool)
        if s == 1:
            loud[:] = True
        elif s > 1:
            for _ in range(max(2, length // 2500)):
                start = int(rng.integers(0, length))
                loud[start:start + int(rng.integers(37, 900))] = True
        x[s] = (sign * np.where(loud, 0.5, 1e-4)).astype(np.float32)
    return x


def _restate(x, y, shift, base, thr, state, block, sub, look, hold, attack, release, hysteresis_db, range_db):
    """The definition, for S streams.  x [S, n], y [S, block] fp32 arrays, shift [S] ints, thr [S] floats, state = (open [S], hold [S] ints,
    gain [S] float32) -> (want [S, block] fp64, new state, level_db [S] fp64, margin_db: how near the nearest fp64 d comes to a threshold)"""
    S, n = x.shape
    nsub = block // sub
    one = np.float32(1.0)
    up, down = one / np.float32(attack), one / np.float32(release)
    floor = np.float32(10.0 ** (range_db / 20.0)) if range_db != -math.inf else np.float32(0.0)
    t = (np.arange(sub, dtype=np.float64) + 1.0) / np.float64(np.float32(sub))
    want = np.empty((S, block), dtype=np.float64)
    new_open, new_hold, new_gain = np.array(state[0]).copy(), np.array(state[1]).copy(), np.array(state[2], dtype=np.float32).copy()
    level = np.empty(S, dtype=np.float64)
    margin = math.inf
    for s in range(S):
        idx = base + int(shift[s]) + np.arange((nsub + look) * sub, dtype=np.int64)
        inside = (idx >= 0) & (idx < n)
        xs = np.where(inside, x[s, np.clip(idx, 0, n - 1)].astype(np.float64), 0.0)
        p = (xs.reshape(nsub + look, sub) ** 2).mean(axis=1)
        th = float(thr[s])
        t_open = 0.0 if th == -math.inf else 10.0 ** (th / 10.0)      # (NaN stays NaN: every comparison with it is false)
        t_close = t_open * 10.0 ** (-hysteresis_db / 10.0)
        is_open, h, g = int(new_open[s]), int(new_hold[s]), np.float32(new_gain[s])
        for i in range(nsub):
            d = p[i:i + look + 1].max()
            if math.isfinite(th):
                d_db = 10.0 * math.log10(d) if d > 0 else -math.inf
                margin = min(margin, abs(d_db - th), abs(d_db - (th - hysteresis_db)))
            if d >= t_open:
                is_open, h = 1, hold
            elif is_open and d >= t_close:
                h = hold
            elif is_open:
                if h > 0:
                    h -= 1
                else:
                    is_open = 0
            tgt = one if is_open else floor
            g_prev = g
            g = min(tgt, np.float32(g + up)) if tgt > g else max(tgt, np.float32(g - down))
            g = np.float32(g)
            ramp = np.float64(g_prev) + (np.float64(g) - np.float64(g_prev)) * t
            want[s, i * sub:(i + 1) * sub] = y[s, i * sub:(i + 1) * sub].astype(np.float64) * ramp
        new_open[s], new_hold[s], new_gain[s] = is_open, h, g
        level[s] = 10.0 * math.log10(max(p[:nsub].mean(), 1e-20))
    return want, (new_open, new_hold, new_gain), level, margin


def _gate(S, block, sub, look, hold, attack, release, range_db=-math.inf, thr=THR, hysteresis_db=HYST):
    from tinyvc_amd.module.infer import StreamGate
    return StreamGate(S, block, threshold_db=thr, hysteresis_db=hysteresis_db, hold_size=hold * sub, attack_size=attack * sub, release_size=release * sub,
                      lookahead_size=look * sub, sub_frame=sub, range_db=range_db, device=DEV)


def _state(gate):
    return gate.open.cpu().numpy().astype(np.int64), gate.hold.cpu().numpy().astype(np.int64), gate.gain.cpu().numpy().copy()


def _check_block(got, y, want, what):
    err = np.abs(got.astype(np.float64) - want)
    bound = SAMPLE_BOUND * np.abs(y.astype(np.float64))
    worst = float((err - bound).max())
    print(f"{what}: max |out - want| / |y| = {float((err / np.maximum(np.abs(y), 1e-30)).max()):.3e} (bound {SAMPLE_BOUND:.3e})")
    assert worst <= 0, f"{what}: a sample is {worst:.3e} past 2^-21 |y|, at (stream, sample) {np.argwhere(err > bound)[0].tolist()}"


def _run_against_restatement(block, sub, look, hold, attack, release, range_db, n, base, shifts, seed, n_blocks=6):
    """n_blocks consecutive blocks of S = len(shifts[0]) streams carrying state; the windows slide over one long signal as a stream's do"""
    eng = _engine()
    S = len(shifts[0])
    sig = _bursts(S, n + (n_blocks - 1) * block, seed)
    ys = torch.randn(n_blocks, S, block, generator=torch.Generator().manual_seed(seed))
    gate = _gate(S, block, sub, look, hold, attack, release, range_db)
    state = _state(gate)
    assert state[0].tolist() == [1] * S and state[1].tolist() == [0] * S and state[2].tolist() == [1.0] * S
    seen_open, seen_closed, seen_ramp, margin = False, False, False, math.inf
    for b in range(n_blocks):
        x = np.ascontiguousarray(sig[:, b * block:b * block + n])
        shift = np.asarray(shifts[b % len(shifts)], dtype=np.int32)
        y = ys[b].numpy()
        out = eng.stream_gate(torch.from_numpy(x).to(DEV), ys[b].to(DEV), torch.from_numpy(shift).to(DEV), gate, base)
        want, state, level, m = _restate(x, y, shift, base, [THR] * S, state, block, sub, look, hold, attack, release, HYST, range_db)
        margin = min(margin, m)
        assert m >= 3.0, f"block {b}: an fp64 d lies {m:.2f} dB from a threshold; the inputs of this test must keep 3 dB"
        got_state = _state(gate)
        what = f"block {block} sub {sub} look {look} hold {hold} attack {attack} release {release} range {range_db}, block {b}"
        assert got_state[0].tolist() == state[0].tolist(), f"{what}: open {got_state[0].tolist()} != {state[0].tolist()}"
        assert got_state[1].tolist() == state[1].tolist(), f"{what}: hold {got_state[1].tolist()} != {state[1].tolist()}"
        assert _same(torch.from_numpy(got_state[2]), torch.from_numpy(state[2])), f"{what}: gain {got_state[2].tolist()} != {state[2].tolist()}"
        lev = gate.level_db.cpu().numpy().astype(np.float64)
        print(f"{what}: max |level_db - want| = {float(np.abs(lev - level).max()):.3e} dB")
        assert np.abs(lev - level).max() <= LEVEL_BOUND_DB, f"{what}: level_db {lev.tolist()} != {level.tolist()}"
        _check_block(out.cpu().numpy(), y, want, what)
        seen_open |= bool(state[0].max() == 1)
        seen_closed |= bool(state[0].min() == 0)
        seen_ramp |= bool(((state[2] > 0) & (state[2] < 1)).any()) or attack == release == 1
    assert seen_open and seen_closed, "the inputs neither opened nor closed a gate"
    return margin, seen_ramp


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------------
SEARCH = 16
SHIFTS = [[0, 1, 3, SEARCH, 2], [SEARCH, 3, 0, 1, 5], [1, 0, SEARCH, 3, 7]]


@pytest.mark.parametrize("range_db", [-math.inf, -20.0], ids=["silence", "minus20"])
@pytest.mark.parametrize("look", [0, 2])
@pytest.mark.parametrize("block,sub", [(480, 120), (1920, 240)])
def test_kernel_equals_the_restatement(block, sub, look, range_db):
    """S = 5, six blocks carrying state, every (hold, attack, release) of {0, 2} x {1, 3} x {1, 4}; planted shifts 0, 1, 3 and `search` (any
    alignment of the window's start).  The window holds everything the gate reads: base + search + block + look * sub <= n."""
    base = 29
    n = base + SEARCH + block + look * sub + 11
    ramps = False
    for k, (hold, attack, release) in enumerate(itertools.product((0, 2), (1, 3), (1, 4))):
        _, r = _run_against_restatement(block, sub, look, hold, attack, release, range_db, n, base, SHIFTS, seed=100 + k)
        ramps |= r and (attack, release) != (1, 1)
    assert ramps, "no gain strictly between the floor and 1 was ever seen"


@pytest.mark.parametrize("base,tail", [(29, -9), (-5, 11), (-100, -9)], ids=["past_the_end", "before_the_start", "both"])
def test_reading_outside_the_window_is_reading_zero(base, tail):
    """base + shift + block + look * sub > n for the streams with the larger shifts (and a < 0 for a negative base): those indices read as 0"""
    block, sub, look = 480, 120, 2
    n = base + SEARCH + block + look * sub + tail
    assert base + SEARCH + block + look * sub > n or base < 0
    _run_against_restatement(block, sub, look, 2, 3, 4, -20.0, n, base, SHIFTS, seed=7)


# ---- 2. open and closed steady states ------------------------------------------------------------------------------------------------------
def test_open_and_closed_steady_states():
    eng = _engine()
    S, block, sub, n = 4, 480, 120, 1200
    x = torch.from_numpy(_bursts(S, n, seed=3)).to(DEV)
    y = torch.randn(S, block, generator=torch.Generator().manual_seed(4)).to(DEV)
    y[0, 5], y[1, 7] = -0.0, 1e-42      # a negative zero and a denormal pass an open gate as they are
    shift = torch.tensor([0, 3, 16, 1], dtype=torch.int32, device=DEV)
    # -inf dB: the ungated stream from its first sample, on every input (stream 0 is floor only)
    gate = _gate(S, block, sub, 2, 2, 3, 4, thr=-math.inf)
    for _ in range(3):
        out = eng.stream_gate(x, y, shift, gate, 40)
        assert _same(out, y), "an open gate changed a bit"
        assert gate.open.tolist() == [1] * S and gate.hold.tolist() == [2] * S and gate.gain.tolist() == [1.0] * S
    # silence (stream 0) under range_db = -inf: closed after hold + release sub-frames, then nothing but zeros
    gate = _gate(S, block, sub, 2, 2, 3, 4)
    outs = [eng.stream_gate(x, y, shift, gate, 40) for _ in range(3)]
    assert gate.open.tolist()[:2] == [0, 1] and gate.gain.tolist()[:2] == [0.0, 1.0]
    assert float(outs[0][0].abs().max()) > 0 and float(outs[2][0].abs().max()) == 0.0, "a long-silent stream does not emit zeros"
    assert _same(outs[2][1], y[1])
    assert abs(float(gate.level_db[0]) + 80.0) < 1e-2 and abs(float(gate.level_db[1]) - 10 * math.log10(0.25)) < 1e-2
    # a NaN threshold keeps a stream closed whatever comes in (stream 1 is loud from end to end), and lets a fresh one close
    gate = _gate(S, block, sub, 2, 2, 3, 4)
    gate.threshold_db[1] = math.nan
    gate.open[1], gate.gain[1] = 0, 0.0
    out = eng.stream_gate(x, y, shift, gate, 40)
    assert gate.open.tolist()[1] == 0 and gate.gain.tolist()[1] == 0.0 and float(out[1].abs().max()) == 0.0
    gate.reset([1])
    assert (gate.open.tolist()[1], gate.hold.tolist()[1], gate.gain.tolist()[1]) == (1, 0, 1.0)
    for _ in range(2):
        out = eng.stream_gate(x, y, shift, gate, 40)
    assert gate.open.tolist()[1] == 0 and float(out[1].abs().max()) == 0.0


# ---- 3. isolation --------------------------------------------------------------------------------------------------------------------------
def _guarded(S, fill, dtype):
    buf = torch.full((S + 2,), fill, dtype=dtype, device=DEV)
    return buf, buf[1:S + 1]


def _guarded_gate(gate):
    """the same gate with every tensor inside guard elements -> (a gate-like object, the guard buffers)"""
    S = gate.n_streams
    bufs = {}
    ns = types.SimpleNamespace(n_streams=S, block_size=gate.block_size, params=gate.params)
    for name, fill, dtype in (("threshold_db", math.nan, torch.float32), ("open", 0x7FC00000, torch.int32), ("hold", 0x7FC00000, torch.int32),
                              ("gain", math.nan, torch.float32), ("level_db", math.nan, torch.float32)):
        bufs[name], view = _guarded(S, fill, dtype)
        view.copy_(getattr(gate, name))
        setattr(ns, name, view)
    return ns, bufs


def _guards_intact(bufs):
    return all(_same(b[[0, -1]], torch.full((2,), math.nan if b.dtype == torch.float32 else 0x7FC00000, dtype=b.dtype)) for b in bufs.values())


def test_streams_are_isolated_and_guards_survive():
    eng = _engine()
    S, block, sub, look, n, base = 5, 480, 120, 2, 1300, 31
    args = (2, 3, 4, -20.0)
    x = torch.from_numpy(_bursts(S, n, seed=11)).to(DEV)
    y = torch.randn(S, block, generator=torch.Generator().manual_seed(12)).to(DEV)
    shift = torch.tensor([0, 1, 3, SEARCH, 2], dtype=torch.int32, device=DEV)
    # NaN guard rows around out, guard elements around the thresholds and the state
    gate, bufs = _guarded_gate(_gate(S, block, sub, look, *args))
    out_buf = torch.full((S + 2, block), math.nan, device=DEV)
    for _ in range(2):
        out = eng.stream_gate(x, y, shift, gate, base, out=out_buf[1:S + 1])
    assert out.data_ptr() == out_buf[1].data_ptr() and bool(out_buf[[0, -1]].isnan().all()) and not bool(out.isnan().any())
    assert _guards_intact(bufs), "a guard element next to the state was written"
    # out aliasing y equals the out-of-place call
    gate2 = _gate(S, block, sub, look, *args)
    yy = y.clone()
    for _ in range(2):
        yy.copy_(y)
        alias = eng.stream_gate(x, yy, shift, gate2, base, out=yy)
    assert alias.data_ptr() == yy.data_ptr() and _same(alias, out)
    assert all(_same(getattr(gate, k), getattr(gate2, k)) for k in ("open", "hold", "gain", "level_db"))
    # a stream alone equals its row of the batch
    for s in range(S):
        g1 = _gate(1, block, sub, look, *args)
        for _ in range(2):
            o1 = eng.stream_gate(x[s:s + 1].contiguous(), y[s:s + 1].contiguous(), shift[s:s + 1].contiguous(), g1, base)
        assert _same(o1[0], out[s]) and _same(g1.gain, gate.gain[s:s + 1].clone()) and g1.open.tolist() == gate.open[s:s + 1].tolist(), f"stream {s}"
    # shift = None is a shift of zeros
    g0, gz = _gate(S, block, sub, look, *args), _gate(S, block, sub, look, *args)
    assert _same(eng.stream_gate(x, y, None, g0, base), eng.stream_gate(x, y, torch.zeros_like(shift), gz, base))
    # a threshold moved between calls moves that stream only: stream 1 (loud from end to end, -6 dB) under a threshold of +10 dB starts to close
    ga, gb = _gate(S, block, sub, look, 0, 3, 4, -20.0), _gate(S, block, sub, look, 0, 3, 4, -20.0)
    eng.stream_gate(x, y, shift, ga, base), eng.stream_gate(x, y, shift, gb, base)
    gb.threshold_db[1] = 10.0
    oa, ob = eng.stream_gate(x, y, shift, ga, base), eng.stream_gate(x, y, shift, gb, base)
    others = [0, 2, 3, 4]
    assert _same(oa[others], ob[others]) and not _same(oa[1], ob[1]) and gb.open.tolist()[1] == 0 and ga.open.tolist()[1] == 1
    assert _same(ga.gain[others], gb.gain[others]) and _same(ga.open[others], gb.open[others])


# ---- 4. what the library refuses -----------------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_header_says():
    eng = _engine()
    S, block, n = 2, 480, 1300
    x = torch.zeros(S, n, device=DEV)
    y = torch.ones(S, block, device=DEV)
    out = torch.full((S, block), 7.0, device=DEV)
    gate = _gate(S, block, 120, 2, 2, 3, 4)
    good = dict(x=x.data_ptr(), n=n, base=0, shift=None, y=y.data_ptr(), out=out.data_ptr(), S=S, block=block, sub=120, look=2, hold=2, attack=3, release=4,
                hysteresis_db=6.0, range_db=-20.0, threshold_db=gate.threshold_db.data_ptr(), open=gate.open.data_ptr(), hold_state=gate.hold.data_ptr(),
                gain=gate.gain.data_ptr(), level_db=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        p = lambda v: ctypes.c_void_p(v) if v is not None else None
        rc = eng.lib.tvc_stream_gate_f32(eng.ctx, eng._stream(), p(a["x"]), a["n"], a["base"], p(a["shift"]), p(a["y"]), p(a["out"]), a["S"], a["block"],
                                         a["sub"], a["look"], a["hold"], a["attack"], a["release"], a["hysteresis_db"], a["range_db"], p(a["threshold_db"]),
                                         p(a["open"]), p(a["hold_state"]), p(a["gain"]), p(a["level_db"]))
        return rc, eng.lib.tvc_last_error(eng.ctx).decode()

    for kw, text in ((dict(sub=250), "sub = 250 is not a multiple of 4"), (dict(sub=128), "not a whole number of 128-sample sub-frames"),
                     (dict(look=4093), "block / sub + look = 4097"), (dict(look=-1), "look = -1 is negative"), (dict(hold=-1), "hold = -1"),
                     (dict(attack=0), "attack = 0"), (dict(release=0), "release = 0"), (dict(block=0), "block = 0 is not positive"),
                     (dict(x=None), "NULL pointer"), (dict(y=None), "NULL pointer"), (dict(out=None), "NULL pointer"), (dict(threshold_db=None), "NULL pointer"),
                     (dict(open=None), "NULL pointer"), (dict(hold_state=None), "NULL pointer"), (dict(gain=None), "NULL pointer"), (dict(S=0), "S <= 0"),
                     (dict(n=0), "n = 0 is outside"), (dict(n=(1 << 40) + 1), "is outside 1 .. 2^40"), (dict(base=(1 << 40) + 1), "above 2^40"),
                     (dict(base=-(1 << 40) - 1), "above 2^40"), (dict(hysteresis_db=-1.0), "hysteresis_db = -1"), (dict(hysteresis_db=math.nan), "hysteresis_db"),
                     (dict(hysteresis_db=math.inf), "hysteresis_db"), (dict(range_db=1.0), "range_db = 1"), (dict(range_db=math.nan), "range_db")):
        rc, err = call(**kw)
        assert rc == -1 and "tvc_stream_gate_f32" in err and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert gate.open.tolist() == [1, 1] and gate.hold.tolist() == [0, 0] and gate.gain.tolist() == [1.0, 1.0]
    rc, _ = call()      # and the well-formed call runs (no level_db, no shift: both are optional)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any())
    # the checked wrapper refuses shapes, dtypes and foreign gates before the library is called
    for a, match in (((x, y[:1].contiguous(), None, gate, 0), "a gate for 2 streams"), ((x, y, torch.zeros(S, device=DEV), gate, 0), "shift must be contiguous int32"),
                     ((x, y, None, gate, 1.5), "base must be an integer"), ((x.double(), y, None, gate, 0), "x must be contiguous fp32"),
                     ((x, y, None, _gate(3, block, 120, 2, 2, 3, 4), 0), "a gate for 3 streams")):
        with pytest.raises(ValueError, match=match):
            eng.stream_gate(*a)


# ---- 5. whole streams ----------------------------------------------------------------------------------------------------------------------
S3 = 3
GEOM = dict(block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3840)      # a window of 4320: nine whole frames
GATE_KW = dict(hold_size=240, attack_size=240, release_size=480, lookahead_size=480, sub_frame=240)
N_BLOCKS = 4


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
    angles = [synth.synth_angle(S3, 9, 700 + i).to(DEV) for i in range(8)]
    mic = torch.from_numpy(_bursts(S3, 8 * 480, seed=21)).to(DEV)
    return tgt, angles, mic


def _stream(gen, tgt, gate=None, use_graph=False, door=None):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=S3, target=tgt, pitch_shift=[0.0, 2.0, -1.5], device=torch.device(DEV), use_graph=use_graph, gate=gate, door=door,
                            **GEOM)
    st.init_buffer()
    return st


def _stream_gate(thr=THR, **kw):
    from tinyvc_amd.module.infer import StreamGate
    args = dict(GATE_KW)
    args.update(kw)
    return StreamGate(S3, 480, threshold_db=thr, hysteresis_db=HYST, device=DEV, **args)


@pytest.fixture(scope="module")
def ungated(gen, model_side):
    """the ungated stream, computed once: per block its output, window, lag and SOLA buffer"""
    tgt, angles, mic = model_side
    st = _stream(gen, tgt)
    rec = []
    for i in range(N_BLOCKS):
        out = st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i])
        rec.append((out.clone(), st.input_wav.clone(), st.last_shift.clone(), st.sola_buffer.clone()))
    assert float(torch.stack([r[0] for r in rec]).abs().max()) > 1e-3, "the ungated stream is silent"
    return rec


def test_a_gate_at_minus_inf_is_the_ungated_stream(gen, model_side, ungated):
    tgt, angles, mic = model_side
    st = _stream(gen, tgt, _stream_gate(-math.inf))
    for i in range(N_BLOCKS):
        out = st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i])
        assert _same(out, ungated[i][0]) and _same(st.last_shift, ungated[i][2]) and _same(st.sola_buffer, ungated[i][3]), f"block {i}"
    assert st.gate.open.tolist() == [1] * S3 and st.gate.gain.tolist() == [1.0] * S3


def test_a_gated_stream_is_the_ungated_one_times_the_restated_gain(gen, model_side, ungated):
    tgt, angles, mic = model_side
    gate = _stream_gate()
    st = _stream(gen, tgt, gate)
    state = _state(gate)
    base = 4320 - 480 - 240 - 240 - 480
    seen = set()
    for i in range(N_BLOCKS):
        out = st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i])
        plain, window, shift, sola = ungated[i]
        # the gate never feeds back: the window, the lag and the SOLA buffer are the ungated stream's, bit for bit
        assert _same(st.input_wav, window) and _same(st.last_shift, shift) and _same(st.sola_buffer, sola), f"block {i}"
        y = plain.cpu().numpy()
        want, state, level, margin = _restate(window.cpu().numpy(), y, shift.cpu().numpy(), base, [THR] * S3, state, 480, 240, 2, 1, 1, 2, HYST, -math.inf)
        assert margin >= 3.0, f"block {i}: an fp64 d lies {margin:.2f} dB from a threshold"
        got = _state(gate)
        assert got[0].tolist() == state[0].tolist() and got[1].tolist() == state[1].tolist() and _same(torch.from_numpy(got[2]), torch.from_numpy(state[2]))
        assert np.abs(gate.level_db.cpu().numpy() - level).max() <= LEVEL_BOUND_DB
        _check_block(out.cpu().numpy(), y, want, f"whole stream, block {i}")
        seen |= set(state[0].tolist())
    assert seen == {0, 1}, "the streams' input neither opened nor closed a gate"


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------------------------
def _run(gen, model_side, use_graph, n_blocks=7):
    tgt, angles, mic = model_side
    gate = _stream_gate()
    st = _stream(gen, tgt, gate, use_graph)
    outs, graphs = [], []
    for i in range(n_blocks):
        if i == 4:
            gate.threshold_db.fill_(-90.0)      # below the floor: everything opens
        if i == 5:
            gate.threshold_db.copy_(torch.tensor([-40.0, 10.0, -40.0]))      # stream 1 is loud (-6 dB): 16 dB under its new threshold
            gate.reset([1])
        outs.append(st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i]).clone())
        graphs.append(st._graph[1][True][0] if use_graph and st._graph is not None and True in st._graph[1] else None)
    return torch.stack(outs), tuple(t.clone() for t in (gate.open, gate.hold, gate.gain, gate.level_db)), graphs, st


def test_graph_replay_equals_eager_with_one_capture(gen, model_side):
    """threshold_db.fill_ / copy_ and gate.reset([1]) between blocks: the graph captured at block 2 replays to the end (the same graph
    object) and equals eager; a gate at another address or with other params() is another key."""
    eager = _run(gen, model_side, False)
    graph = _run(gen, model_side, True)
    g = graph[2]
    assert g[0] is None and g[1] is None and g[2] is not None and all(x is g[2] for x in g[2:]), "a threshold / a reset captured a new graph"
    assert _same(eager[0], graph[0]), "graph replay is not sample-exact"
    assert all(_same(a, b) for a, b in zip(eager[1], graph[1])), "the final gate state differs"
    assert not _same(eager[0][4], eager[0][3]) and eager[1][0].tolist()[0] == 0 and eager[1][0].tolist()[1] == 0      # thresholds took effect
    st = graph[3]
    key = st._graph_key()
    assert key == st._graph[0]
    old = st.gate
    st.gate = _stream_gate()      # the same parameters at another address
    assert st._graph_key() != key
    for kw in (dict(hold_size=480), dict(attack_size=480), dict(release_size=240), dict(lookahead_size=240), dict(sub_frame=120), dict(range_db=-20.0)):
        twin = _stream_gate(**kw)
        for name in ("threshold_db", "open", "hold", "gain", "level_db"):      # the same addresses: only params() tell them apart
            setattr(twin, name, getattr(old, name))
        st.gate = twin
        assert st._graph_key() != key, f"{kw} did not change the graph key"
    twin = _stream_gate()
    for name in ("threshold_db", "open", "hold", "gain", "level_db"):
        setattr(twin, name, getattr(old, name))
    st.gate = twin
    assert st._graph_key() == key, "values, not addresses or params(), went into the key"
    # a new gate on the same stream: the next block captures anew
    st.gate = _stream_gate()
    tgt, angles, mic = model_side
    st.audio_callback(mic[:, :480], noise_angle=angles[0])
    assert st._graph[1][True][0] is not g[2]


# ---- 7. the door and the entry script ------------------------------------------------------------------------------------------------------
def test_through_a_door_the_gate_sits_between_the_block_and_the_way_out(gen, model_side):
    from tinyvc_amd.module.infer import StreamDoor
    tgt, angles, mic = model_side
    eng = gen.engine(torch.device(DEV))
    pcm = (torch.from_numpy(_bursts(S3, N_BLOCKS * 960, seed=33, period=14)) * 32767).to(torch.int16).to(DEV)
    door = StreamDoor(S3, 48000, block_size=480, input_gain=-1.0, output_gain=2.0, device=DEV)
    st = _stream(gen, tgt, _stream_gate(), door=door)
    hand_door = StreamDoor(S3, 48000, block_size=480, input_gain=-1.0, output_gain=2.0, device=DEV)
    hand_door.prepare(eng)
    hand = _stream(gen, tgt, _stream_gate())
    closed = False
    for i in range(N_BLOCKS):
        blk = pcm[:, i * 960:(i + 1) * 960]
        got = st.audio_callback_pcm(blk, noise_angle=angles[i])
        want = hand_door.pull(eng, hand.audio_callback(hand_door.push(eng, blk), noise_angle=angles[i]))
        assert got.dtype == torch.int16 and _same(got, want), f"block {i}"
        assert all(_same(getattr(st.gate, k), getattr(hand.gate, k)) for k in ("open", "hold", "gain", "level_db"))
        closed |= 0 in st.gate.open.tolist()
    assert closed, "no gate closed: the test would pass without one"


E2E_BLOCKS = 8


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The recording: loud for its first 3000 samples, floor after.  At the default geometry the gate of block b looks at the input from
    (b - 4) * 1920 + shift on, shift in [0, 1920]: blocks 0 .. 3 see the zeros the window starts with (the gate closes), block 4 sees the
    burst and the 50 ms hold keeps it open to its end (its last sub-frame starts before 3600 < 3000 + 1200), block 7 starts past 5760 (closed)."""
    d = tmp_path_factory.mktemp("gate")
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(500, seed=2), d / "index.pt")
    t = torch.arange(E2E_BLOCKS * 1920)
    mic = torch.where((t // 7) % 2 == 0, 1.0, -1.0) * torch.where(t < 3000, 0.45, 9e-5)
    audio_io.save(str(d / "mic.wav"), mic[None], 24000)
    common = ["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "index.pt"), "--input-wav", str(d / "mic.wav"), "--streams", "2",
              "-d", DEV, "-p", "0.5", "-og", "1.5"]
    return d, common


def test_infer_streaming_gate_writes_what_the_class_loop_produces(files, capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor, StreamGate
    d, common = files
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--gate", "-40", "--gate-hold", "52", "--gate-release", "30", "--output-wav", str(d / "gate.wav")]) == 0
    text = capsys.readouterr().out
    assert "Noise gate at -40 dB (hysteresis 6 dB, range -inf dB): hold 50 ms, attack 10 ms, release 30 ms, look-ahead 20 ms in 10 ms sub-frames" in text
    assert "stream 0: gate open at the end of " in text and f"of {E2E_BLOCKS} blocks" in text and "p50" in text
    torch.manual_seed(3)
    dev = torch.device(DEV)
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), dev)
    door = StreamDoor(2, 24000, block_size=1920, output_gain=1.5, device=dev)
    gate = StreamGate(2, 1920, threshold_db=-40.0, hysteresis_db=6.0, hold_size=1200, attack_size=240, release_size=720, lookahead_size=480, device=dev)
    st = BatchedStreamInfer(gen, n_streams=2, pitch_shift=0.5, block_size=1920, device=dev, extra_size=3840, door=door, gate=gate)
    st.target = torch.load(d / "index.pt").to(dev)
    st.init_buffer()
    outs, n_open = [], 0
    for blk in infer_streaming.int16_blocks_from_wav(str(d / "mic.wav"), 24000, 1920, gen.engine(dev)):
        pcm = torch.from_numpy(np.ascontiguousarray(blk)).to(dev)
        outs.append(st.audio_callback_pcm(pcm.expand(2, -1)).cpu().numpy()[0])
        n_open += gate.open.tolist()[0]
    assert len(outs) == E2E_BLOCKS and 0 < n_open < E2E_BLOCKS, "the recording neither opened nor closed the gate"
    assert f"stream 0: gate open at the end of {n_open} of {E2E_BLOCKS} blocks" in text
    audio_io.save(str(d / "want.wav"), torch.from_numpy(np.concatenate(outs).astype(np.float32) / 32768)[None], 24000)
    assert open(d / "gate.wav", "rb").read() == open(d / "want.wav", "rb").read()
    # and without --gate the script runs the stream it has always run: another file
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--output-wav", str(d / "plain.wav")]) == 0
    assert "Noise gate" not in capsys.readouterr().out and open(d / "plain.wav", "rb").read() != open(d / "gate.wav", "rb").read()
