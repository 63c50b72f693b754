"""The loudness envelope match on the GPU (tvc_loudness_match_f32, tvc_stream_loudness_f32; the definition is in include/tinyvc_hip.h)
against its fp64 restatement (helpers_loudness).

Bounds.  A gain is one fp64 value rounded to fp32 once; the kernel's and the restatement's fp64 values differ by the order of their fp64
sums and by the last bits of log2 / exp2 - about 1e-13 relative - so the two roundings differ only where that value lies within 1e-13 of an
fp32 rounding boundary: the gains are held to 1 fp32 ulp.  The samples are fp32 operations rounded one by one, so they are held, bit for
bit, to the numpy ramp of the kernel's OWN gains.  The rings are fp64 sums of up to 240 exact squares in two orders: 1e-12 relative.
Everything the header calls independent (block cuts, S, neighbours, out == y, a ragged row against its own call) is held bit for bit."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import helpers_loudness as H
from helpers import state_dicts
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUB = 240


def _engine():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _bits(x):
    x = torch.as_tensor(x).cpu().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else (x.view(torch.int64) if x.dtype == torch.float64 else x)


def _same(a, b):
    """bit for bit (torch.equal would call -0.0 and 0.0 equal and a NaN unequal to itself)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _settings(smooth=2, sub=SUB, floor_db=-60.0, boost_db=12.0, cut_db=40.0):
    return types.SimpleNamespace(sub_frame=sub, smooth=smooth, floor_db=floor_db, boost_db=boost_db, cut_db=cut_db)


def _signal(rows, nsub, seed, sub=SUB):
    """[rows, nsub * sub] fp32 noise under an envelope that moves from sub-frame to sub-frame between -70 and -6 dB: both caps, the floor
    and everything between them are reached"""
    rng = np.random.default_rng(seed)
    env = 10.0 ** (rng.uniform(-70.0, -6.0, size=(rows, nsub)) / 20.0)
    return (rng.standard_normal((rows, nsub, sub)) * env[:, :, None]).reshape(rows, nsub * sub).astype(np.float32)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype).to(DEV).contiguous()


@pytest.fixture(scope="module")
def tile():
    from tinyvc_amd.engine import loudness_geometry
    return loudness_geometry(SUB * 1000, SUB, 2)[2]


# ---- 1. the offline stage ------------------------------------------------------------------------------------------------------------------
SHARES = [1.0, 0.6, 0.3]


def _offline_case(tile, smooth, ragged):
    """B = 3 over three tiles and a bit: the equal batch ends smooth + 1 sub-frames past a tile edge, the ragged rows 0, 1 and `smooth` past it"""
    nmax = 3 * tile + smooth + 1
    lens = [(3 * tile + d) * SUB for d in (0, 1, smooth)] if ragged else None
    return _signal(3, nmax, 11 + smooth), _signal(3, nmax, 12 + smooth), lens


@pytest.mark.parametrize("ragged", [False, True], ids=["equal", "ragged"])
@pytest.mark.parametrize("smooth", [2, 0])
def test_offline_gains_within_an_ulp_and_samples_from_the_kernels_own_gains(tile, smooth, ragged):
    eng = _engine()
    x, y, lens = _offline_case(tile, smooth, ragged)
    out, gains = eng.loudness_match(_dev(x), _dev(y), _dev(SHARES), lengths=lens, settings=_settings(smooth), want_gains=True)
    out, gains = out.cpu().numpy(), gains.cpu().numpy()
    assert gains.shape == (3, x.shape[1] // SUB + 1)
    moved = 0
    for b in range(3):
        n = lens[b] if ragged else x.shape[1]
        want = H.offline_edges(x[b], y[b], SHARES[b], length=n, smooth=smooth)
        d = H.ulps(gains[b], want)
        print(f"smooth {smooth} {'ragged' if ragged else 'equal'} row {b}: gains {d} ulp from the restatement, {gains[b].min():.4g} .. {gains[b].max():.4g}")
        assert d <= 1, f"row {b}: {d} ulp"
        assert _same(out[b, :n], H.ramp(y[b, :n], gains[b, :n // SUB + 1], SUB)), f"row {b}: the samples are not the fp32 ramp of the kernel's own gains"
        assert _same(out[b, n:], y[b, n:]) and bool((gains[b, n // SUB + 1:] == 1.0).all()), f"row {b}: behind its length"
        moved += int((gains[b] != 1.0).sum())
    assert moved > 3 * tile, "the gains hardly moved: the case would pass without the stage"


def test_offline_share_zero_aliasing_and_a_ragged_row_alone(tile):
    eng = _engine()
    x, y, lens = _offline_case(tile, 2, True)
    X, Y = _dev(x), _dev(y)
    zero = eng.loudness_match(X, Y, _dev([0.0, 0.0, 0.0]), settings=_settings())
    assert _same(zero, Y), "share 0 changed a bit"
    for bad in (math.nan, -3.0):      # NaN is 0, values below 0 are clamped to it
        assert _same(eng.loudness_match(X, Y, _dev([bad] * 3), settings=_settings()), Y)
    over, g_over = eng.loudness_match(X, Y, _dev([7.0] * 3), settings=_settings(), want_gains=True)      # ... and above 1 to 1
    one, g_one = eng.loudness_match(X, Y, _dev([1.0] * 3), settings=_settings(), want_gains=True)
    assert _same(over, one) and _same(g_over, g_one)
    mixed, g_mixed = eng.loudness_match(X, Y, _dev([1.0, 0.0, 0.3]), lengths=lens, settings=_settings(), want_gains=True)
    assert _same(mixed[1], Y[1]) and bool((g_mixed[1] == 1.0).all()) and not _same(mixed[0], Y[0]) and not _same(mixed[2], Y[2])
    for ln, smooth in ((None, 2), (lens, 2), (lens, 32)):      # smooth = 32: the powers an in-place walk carries from tile to tile are more than a tile
        apart, g_apart = eng.loudness_match(X, Y, _dev(SHARES), lengths=ln, settings=_settings(smooth), want_gains=True)
        inplace = Y.clone()
        res, g_in = eng.loudness_match(X, inplace, _dev(SHARES), lengths=ln, settings=_settings(smooth), out=inplace, want_gains=True)
        assert res is inplace and _same(inplace, apart) and _same(g_in, g_apart), "out = y gives other bits"
    assert H.ulps(g_apart[0, :lens[0] // SUB + 1].cpu().numpy(), H.offline_edges(x[0], y[0], SHARES[0], length=lens[0], smooth=32)[:lens[0] // SUB + 1]) <= 1
    ragged, g_ragged = eng.loudness_match(X, Y, _dev(SHARES), lengths=lens, settings=_settings(), want_gains=True)
    for b in range(3):
        n = lens[b]
        alone, g_alone = eng.loudness_match(X[b:b + 1, :n].contiguous(), Y[b:b + 1, :n].contiguous(), _dev(SHARES[b:b + 1]), settings=_settings(), want_gains=True)
        assert _same(ragged[b, :n], alone[0]) and _same(g_ragged[b, :n // SUB + 1], g_alone[0]), f"row {b} is not its own B = 1 call"
    assert _same(eng.loudness_match(X, Y, _dev(SHARES), lengths=torch.tensor(lens), settings=_settings()), ragged)      # (a host tensor is a host sequence)


def test_offline_more_rows_than_one_launch_carries_lengths_for():
    """the lengths travel as kernel arguments, 384 rows to a launch: 390 short ragged rows, apart and in place, every row against its own call
    where the launches meet and at both ends"""
    eng = _engine()
    B, n = 390, 6
    x, y = _signal(B, n, 45), _signal(B, n, 46)
    lens = [(1 + (b * 5) % n) * SUB for b in range(B)]
    share = _dev(np.linspace(0.2, 1.0, B))
    X, Y = _dev(x), _dev(y)
    out, gains = eng.loudness_match(X, Y, share, lengths=lens, settings=_settings(1), want_gains=True)
    inplace = Y.clone()
    eng.loudness_match(X, inplace, share, lengths=lens, settings=_settings(1), out=inplace)
    assert _same(inplace, out)
    for b in (0, 1, 382, 383, 384, 385, 389):
        m = lens[b]
        alone, g_alone = eng.loudness_match(X[b:b + 1, :m].contiguous(), Y[b:b + 1, :m].contiguous(), share[b:b + 1].contiguous(), settings=_settings(1), want_gains=True)
        assert _same(out[b, :m], alone[0]) and _same(gains[b, :m // SUB + 1], g_alone[0]) and _same(out[b, m:], Y[b, m:]), f"row {b}"
        assert H.ulps(g_alone[0].cpu().numpy(), H.offline_edges(x[b, :m], y[b, :m], float(share[b]), smooth=1)) <= 1


def test_offline_planted_cases(tile):
    eng = _engine()
    n = 2 * tile + 3
    loud, silent = np.where(_signal(1, n, 31)[0] > 0, np.float32(0.25), np.float32(-0.25)), np.zeros(n * SUB, np.float32)      # a power of 1 / 16
    one = _dev([1.0])

    def run(x, y, share=one, **kw):
        out, gains = eng.loudness_match(_dev(x[None]), _dev(y[None]), share, settings=_settings(**kw), want_gains=True)
        return out[0].cpu().numpy(), gains[0].cpu().numpy()

    out, gains = run(silent, silent)
    assert bool((gains == 1.0).all()) and _same(out, silent), "silence under silence"
    out, gains = run(loud, silent)
    assert bool((gains == np.float32(10.0 ** (12.0 / 20.0))).all()) and _same(out, silent), "y silent under a loud x: the rounded boost cap"
    out, gains = run(silent, loud)
    assert bool((gains == np.float32(10.0 ** (-40.0 / 20.0))).all()) and _same(out, H.ramp(loud, gains, SUB)), "x silent under a loud y: the rounded cut cap"
    out, gains = run(loud, silent, boost_db=0.0)
    assert bool((gains == 1.0).all()), "boost_db = 0 never turns up"
    # y = x / 4: the ratio of the envelopes is exactly 16 in every window
    x = _signal(1, n, 32)[0] * np.float32(30.0)      # -40 .. +23 dB: every power, and a sixteenth of it, above the floor
    for e, want in ((1.0, 4.0), (0.5, 2.0)):
        out, gains = run(x, x / np.float32(4.0), _dev([e]), boost_db=20.0)
        d = H.ulps(gains, np.full_like(gains, want))
        print(f"y = x / 4, e = {e}: gains {d} ulp from {want}")
        assert d <= 1
    # one NaN and one Inf sample in x: gain 1 on exactly the sub-frames whose window holds it, the others as ever
    x, y = _signal(1, n, 33)[0], _signal(1, n, 34)[0]
    k_nan, k_inf = tile - 1, tile + 9      # the NaN's window straddles a tile edge
    x[k_nan * SUB + 7], x[k_inf * SUB + 200] = np.nan, np.inf
    out, gains = run(x, y)
    want = H.offline_edges(x, y, 1.0)
    hit = np.zeros(n, bool)
    for k in (k_nan, k_inf):
        hit[k - 2:k + 3] = True
    assert bool((gains[1:][hit] == 1.0).all()) and bool((want[1:][~hit] != 1.0).all()) and bool((gains[1:][~hit] != 1.0).all())
    assert H.ulps(gains, want) <= 1 and _same(out, H.ramp(y, gains, SUB))
    # ... and likewise in y
    x, y = _signal(1, n, 35)[0], _signal(1, n, 36)[0]
    y[5 * SUB + 1] = np.inf
    out, gains = run(x, y)
    assert bool((gains[1:][3:8] == 1.0).all()) and gains[3] != 1.0 and gains[9] != 1.0 and H.ulps(gains, H.offline_edges(x, y, 1.0)) <= 1


def test_offline_five_minute_row():
    """30 000 sub-frames in one row (7.2 million samples, 469 tiles), apart and in place: 64-bit indexing and the walk over a long row"""
    eng = _engine()
    n = 30000
    x, y = _signal(1, n, 41), _signal(1, n, 42)
    X, Y = _dev(x), _dev(y)
    out, gains = eng.loudness_match(X, Y, _dev([0.8]), settings=_settings(), want_gains=True)
    want = H.offline_edges(x[0], y[0], 0.8)
    d = H.ulps(gains[0].cpu().numpy(), want)
    print(f"five-minute row: gains {d} ulp from the restatement")
    assert d <= 1 and _same(out[0], H.ramp(y[0], gains[0].cpu().numpy(), SUB))
    res = eng.loudness_match(X, Y, _dev([0.8]), settings=_settings(), out=Y)
    assert res is Y and _same(Y, out)


def test_offline_refusals_through_the_c_abi(tile):
    eng = _engine()
    B, L = 2, 4 * SUB
    x, y = torch.zeros(B, L, device=DEV), torch.ones(B, L, device=DEV)
    out = torch.full((B, L), 7.0, device=DEV)
    share = torch.ones(B, device=DEV)
    good = dict(x=x.data_ptr(), y=y.data_ptr(), out=out.data_ptr(), B=B, L=L, lengths=None, share=share.data_ptr(), sub=SUB, smooth=2, floor_db=-60.0, boost_db=12.0,
                cut_db=40.0, gains=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        p = lambda v: ctypes.c_void_p(v) if v is not None else None
        rc = eng.lib.tvc_loudness_match_f32(eng.ctx, eng._stream(), p(a["x"]), p(a["y"]), p(a["out"]), a["B"], a["L"], p(a["lengths"]), p(a["share"]), a["sub"],
                                            a["smooth"], a["floor_db"], a["boost_db"], a["cut_db"], p(a["gains"]))
        return rc, eng.lib.tvc_last_error(eng.ctx).decode()

    for kw, text in ((dict(sub=250), "sub = 250 is not a multiple of 4"), (dict(sub=2), "sub = 2 is outside 4 .. 65536"), (dict(sub=256), "not a whole number of 256-sample"),
                     (dict(L=0), "length = 0 is outside"), (dict(smooth=33), "smooth = 33 is outside 0 .. 32"), (dict(smooth=-1), "smooth = -1"),
                     (dict(x=None), "NULL pointer"), (dict(y=None), "NULL pointer"), (dict(out=None), "NULL pointer"), (dict(share=None), "NULL pointer"),
                     (dict(B=0), "B <= 0"), (dict(floor_db=math.nan), "floor_db = nan is not finite"), (dict(floor_db=-math.inf), "floor_db = -inf is not finite"),
                     (dict(floor_db=-1e30), "is not a positive finite double"), (dict(boost_db=-1.0), "boost_db = -1 is not a finite number >= 0"),
                     (dict(boost_db=math.inf), "boost_db = inf"), (dict(boost_db=math.nan), "boost_db = nan"), (dict(boost_db=1000.0), "is not a finite fp32 number"),
                     (dict(cut_db=-0.5), "cut_db = -0.5 is not a finite number >= 0"), (dict(cut_db=math.nan), "cut_db = nan"), (dict(cut_db=2000.0), "is not a positive fp32 number"),
                     (dict(x=x.data_ptr() + 4), "16-byte aligned"), (dict(out=y.data_ptr() + 16 * SUB), "out overlaps x, or y without being y"),
                     (dict(out=x.data_ptr()), "out overlaps x")):
        rc, err = call(**kw)
        assert rc == -1 and "tvc_loudness_match_f32" in err and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any())
    for a, kw, match in (((x, y[:1].contiguous(), share), {}, "must have one shape"), ((x.double(), y, share), {}, "x must be contiguous fp32"),
                         ((x, y, share[:1]), {}, "share must be contiguous fp32 \\[2\\]"), ((x, y, share), dict(lengths=[SUB]), "lengths: a host sequence of one integer per row"),
                         ((x, y, share), dict(lengths=torch.tensor([SUB, SUB], device=DEV)), "lengths: a host sequence"), ((x, y, share), dict(lengths=[SUB, 2.5]), "lengths: a host sequence"),
                         ((x, y, share), dict(lengths=[SUB, SUB + 1]), "whole number of 240-sample sub-frames"), ((x, y, share), dict(out=out[:1]), "out must be contiguous fp32"),
                         ((x, y, share), dict(settings=_settings(smooth=40)), "smooth = 40 is outside"), ((x, y, share), dict(settings=_settings(cut_db=-1.0)), "cut_db")):
        with pytest.raises(ValueError, match=match):
            eng.loudness_match(*a, **kw)


# ---- 2. the stream stage -------------------------------------------------------------------------------------------------------------------
S3 = 3
STREAM_SHARES = [1.0, 0.55, 0.9]


def _stage(S, block, smooth, share=1.0, **kw):
    from tinyvc_amd.module.infer import StreamLoudness
    return StreamLoudness(S, block, share=share, sub_frame=SUB, smooth=smooth, device=DEV, **kw)


def _state(stage):
    return {k: getattr(stage, k).cpu().clone() for k in ("src_ring", "out_ring", "frames", "gain", "gain_db")}


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rel * np.abs(want)).all())


def _stream_inputs(block, n, seed, n_blocks=6):
    """per block: windows [S3, n], emitted blocks [S3, block], lags [S3] that move per block and per stream, and a base; the first and the
    last two blocks reach outside the window - in front of its start, behind its end, and both"""
    rng = np.random.default_rng(seed)
    room = n - block
    blocks = []
    for i in range(n_blocks):
        base = (-SUB - 17, room // 2, room // 3, room // 2 + 5, room + 50, -block // 2)[i % 6]
        shift = rng.integers(0, 200, size=S3).astype(np.int32)
        win = _signal(S3, -(-n // SUB), seed * 100 + i)[:, :n].copy()
        if i == n_blocks - 1:
            win = win[:, :block + 100].copy()      # a window shorter than what the block reaches for on both sides
        blocks.append((win, _signal(S3, block // SUB, seed * 100 + 50 + i), shift, base))
    return blocks


@pytest.mark.parametrize("block,smooth", [(480, 2), (1920, 0), (1920, 2)], ids=["b480_w5", "b1920_w1", "b1920_w5"])
def test_stream_equals_the_restatement_and_its_own_single_stream_call(block, smooth):
    eng = _engine()
    stage = _stage(S3, block, smooth, share=STREAM_SHARES)
    alone = [_stage(1, block, smooth, share=STREAM_SHARES[s]) for s in range(S3)]
    refs = [H.StreamRestatement(SUB, smooth) for _ in range(S3)]
    outside = set()
    for i, (win, y, shift, base) in enumerate(_stream_inputs(block, 2 * block + 700, 7 + smooth)):
        W, Y, SH = _dev(win), _dev(y), _dev(shift, torch.int32)
        out, gains = eng.stream_loudness(W, Y, SH, stage, base, want_gains=True)
        st = _state(stage)
        for s in range(S3):
            a = base + int(shift[s])
            outside |= ({"front"} if a < 0 else set()) | ({"back"} if a + block > win.shape[1] else set())
            want = refs[s].block(win[s], y[s], a, STREAM_SHARES[s])
            got = gains[s].cpu().numpy()
            d = H.ulps(got, want)
            print(f"block {block} smooth {smooth} #{i} stream {s}: gains {d} ulp from the restatement")
            assert d <= 1, f"block {i} stream {s}: {d} ulp"
            assert _same(out[s], H.ramp(y[s], got, SUB)), f"block {i} stream {s}: the samples are not the ramp of the kernel's own gains"
            assert int(st["frames"][s]) == refs[s].frames and _same(st["gain"][s], gains[s, -1].cpu()) and H.ulps(st["gain"][s:s + 1].numpy(), [refs[s].gain]) <= 1
            assert _close(st["src_ring"][s], refs[s].src_ring, 1e-12) and _close(st["out_ring"][s], refs[s].out_ring, 1e-12), f"block {i} stream {s}: rings"
            assert abs(float(st["gain_db"][s]) - 20.0 * math.log10(float(st["gain"][s]))) <= 1e-4
            o1, g1 = eng.stream_loudness(W[s:s + 1].contiguous(), Y[s:s + 1].contiguous(), SH[s:s + 1].contiguous(), alone[s], base, want_gains=True)
            a1 = _state(alone[s])
            assert _same(o1[0], out[s]) and _same(g1[0], gains[s]) and all(_same(a1[k][0], st[k][s]) for k in st), f"block {i}: row {s} is not its S = 1 call"
    assert outside == {"front", "back"}, "no block reached outside its window at both ends"


def test_stream_cut_into_blocks_and_against_the_offline_gains():
    """one signal at lag 0 cut into 480-, 960- and 1920-sample blocks: identical samples, rings, count and gain; and the stream's gain of
    sub-frame i is the offline gain of sub-frame i - smooth wherever both windows are whole"""
    eng = _engine()
    total, smooth = 3840, 2
    x, y = _signal(2, total // SUB, 51), _signal(2, total // SUB, 52)
    runs = {}
    for block in (480, 960, 1920):
        stage = _stage(2, block, smooth, share=[1.0, 0.4])
        outs, gains = [], []
        for i in range(0, total, block):
            o, g = eng.stream_loudness(_dev(x[:, i:i + block]), _dev(y[:, i:i + block]), None, stage, 0, want_gains=True)
            outs.append(o)
            gains.append(g[:, 1:])
        runs[block] = (torch.cat(outs, 1), torch.cat(gains, 1), _state(stage))
    for block in (960, 1920):
        assert _same(runs[block][0], runs[480][0]) and _same(runs[block][1], runs[480][1]), f"{block}-sample blocks give other samples"
        assert all(_same(runs[block][2][k], runs[480][2][k]) for k in runs[480][2]), f"{block}-sample blocks leave another state"
    assert runs[480][2]["frames"].tolist() == [16, 16]
    _, off = eng.loudness_match(_dev(x), _dev(y), _dev([1.0, 0.4]), settings=_settings(smooth), want_gains=True)
    stream = runs[480][1]      # [2, 16]: the gain of stream sub-frame i (its edge i + 1)
    n = total // SUB
    assert _same(stream[:, 2 * smooth:], off[:, smooth + 1:n - smooth + 1]), "the stream is not the offline gain sequence `smooth` sub-frames late"
    assert not _same(stream[:, :2 * smooth], off[:, 1:2 * smooth + 1])      # (before that the windows differ)


def test_stream_block_longer_than_the_kernels_chunk():
    """700 sub-frames in one block (the kernel keeps 512 powers at a time) against seven blocks of 100: the same bits, and the restatement"""
    from tinyvc_amd.module.infer import StreamLoudness
    eng = _engine()
    sub, smooth, total = 4, 3, 2800
    x, y = _signal(2, total // sub, 55, sub), _signal(2, total // sub, 56, sub)
    runs = {}
    for block in (400, 2800):
        stage = StreamLoudness(2, block, share=[1.0, 0.7], sub_frame=sub, smooth=smooth, device=DEV)
        outs, gains = [], []
        for i in range(0, total, block):
            o, g = eng.stream_loudness(_dev(x[:, i:i + block]), _dev(y[:, i:i + block]), None, stage, 0, want_gains=True)
            outs.append(o)
            gains.append(g[:, 1:])
        runs[block] = (torch.cat(outs, 1), torch.cat(gains, 1), _state(stage))
    assert _same(runs[2800][0], runs[400][0]) and _same(runs[2800][1], runs[400][1]) and all(_same(runs[2800][2][k], runs[400][2][k]) for k in runs[400][2])
    assert runs[2800][2]["frames"].tolist() == [700, 700]
    for s, e in enumerate((1.0, 0.7)):
        ref = H.StreamRestatement(sub, smooth)
        want = ref.block(x[s], y[s], 0, e)
        assert H.ulps(runs[2800][1][s].cpu().numpy(), want[1:]) <= 1 and _same(runs[2800][0][s], H.ramp(y[s], np.concatenate([want[:1], runs[2800][1][s].cpu().numpy()]), sub))


def test_stream_share_zero_reset_and_silence():
    eng = _engine()
    block, smooth = 480, 2
    blocks = _stream_inputs(block, 1700, 61, n_blocks=4)
    warm, cold = _stage(S3, block, smooth, share=0.0), _stage(S3, block, smooth, share=1.0)
    for win, y, shift, base in blocks[:3]:
        out = eng.stream_loudness(_dev(win), _dev(y), _dev(shift, torch.int32), warm, base)
        assert _same(out, _dev(y)), "share 0 changed a bit"
        eng.stream_loudness(_dev(win), _dev(y), _dev(shift, torch.int32), cold, base)
    sw, sc = _state(warm), _state(cold)
    assert sw["frames"].tolist() == [6] * S3 and _same(sw["src_ring"], sc["src_ring"]) and _same(sw["out_ring"], sc["out_ring"]), "share 0 did not advance the state"
    assert sw["gain"].tolist() == [1.0] * S3 and sw["gain_db"].tolist() == [0.0] * S3 and float(sw["src_ring"].abs().max()) > 0
    # raising the share starts from the warm envelope: the next block's gains are those of the stream that ran at share 1 all along
    win, y, shift, base = blocks[3]
    warm.share.fill_(1.0)
    twin = _stage(S3, block, smooth, share=1.0)      # for the reset below: cold's history, kept whole
    for k in ("src_ring", "out_ring", "frames", "gain", "gain_db"):
        getattr(twin, k).copy_(getattr(cold, k))
    _, gw = eng.stream_loudness(_dev(win), _dev(y), _dev(shift, torch.int32), warm, base, want_gains=True)
    cold.reset([1])
    oc, gc = eng.stream_loudness(_dev(win), _dev(y), _dev(shift, torch.int32), cold, base, want_gains=True)
    ot, gt = eng.stream_loudness(_dev(win), _dev(y), _dev(shift, torch.int32), twin, base, want_gains=True)
    assert _same(gw[:, 1:], gt[:, 1:]) and _same(gw[:, 0], torch.ones(S3, device=DEV)), "the warm envelope was not used"
    # reset([1]) restarts stream 1 only
    fresh = _stage(1, block, smooth, share=1.0)
    of, gf = eng.stream_loudness(_dev(win[1:2]), _dev(y[1:2]), _dev(shift[1:2], torch.int32), fresh, base, want_gains=True)
    assert _same(oc[[0, 2]], ot[[0, 2]]) and _same(gc[[0, 2]], gt[[0, 2]]) and _same(oc[1], of[0]) and _same(gc[1], gf[0]) and not _same(gc[1], gt[1])
    sc, sf = _state(cold), _state(fresh)
    assert sc["frames"].tolist() == [8, 2, 8] and all(_same(sc[k][1], sf[k][0]) for k in sc)
    # an all-zero block moves no gain away from 1
    quiet = _stage(S3, block, smooth, share=1.0)
    zeros = torch.zeros(S3, block, device=DEV)
    for _ in range(2):
        out, g = eng.stream_loudness(torch.zeros(S3, 1700, device=DEV), zeros, None, quiet, 300, want_gains=True)
        assert bool((g == 1.0).all()) and _same(out, zeros)
    assert quiet.gain.tolist() == [1.0] * S3 and quiet.frames.tolist() == [4] * S3


def test_stream_refusals_through_the_c_abi():
    eng = _engine()
    S, block, n = 2, 480, 1300
    x, y = torch.zeros(S, n, device=DEV), torch.ones(S, block, device=DEV)
    out = torch.full((S, block), 7.0, device=DEV)
    stage = _stage(S, block, 2)
    good = dict(x=x.data_ptr(), n=n, base=0, shift=None, y=y.data_ptr(), out=out.data_ptr(), S=S, block=block, sub=SUB, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0,
                share=stage.share.data_ptr(), src_ring=stage.src_ring.data_ptr(), out_ring=stage.out_ring.data_ptr(), frames=stage.frames.data_ptr(),
                gain=stage.gain.data_ptr(), gain_db=None, gains=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        p = lambda v: ctypes.c_void_p(v) if v is not None else None
        rc = eng.lib.tvc_stream_loudness_f32(eng.ctx, eng._stream(), p(a["x"]), a["n"], a["base"], p(a["shift"]), p(a["y"]), p(a["out"]), a["S"], a["block"], a["sub"],
                                             a["smooth"], a["floor_db"], a["boost_db"], a["cut_db"], p(a["share"]), p(a["src_ring"]), p(a["out_ring"]), p(a["frames"]),
                                             p(a["gain"]), p(a["gain_db"]), p(a["gains"]))
        return rc, eng.lib.tvc_last_error(eng.ctx).decode()

    for kw, text in ((dict(sub=250), "sub = 250 is not a multiple of 4"), (dict(sub=128), "not a whole number of 128-sample sub-frames"),
                     (dict(block=4097 * 4, sub=4), "block / sub = 4097 sub-frames is above 4096"), (dict(block=0), "length = 0 is outside"),
                     (dict(smooth=33), "smooth = 33 is outside 0 .. 32"), (dict(x=None), "NULL pointer"), (dict(y=None), "NULL pointer"), (dict(out=None), "NULL pointer"),
                     (dict(share=None), "NULL pointer"), (dict(src_ring=None), "NULL pointer"), (dict(out_ring=None), "NULL pointer"), (dict(frames=None), "NULL pointer"),
                     (dict(gain=None), "NULL pointer"), (dict(S=0), "S <= 0"), (dict(n=0), "n = 0 is outside"), (dict(base=(1 << 40) + 1), "above 2^40"),
                     (dict(floor_db=math.nan), "floor_db = nan is not finite"), (dict(boost_db=-1.0), "boost_db = -1"), (dict(boost_db=math.inf), "boost_db = inf"),
                     (dict(cut_db=-1.0), "cut_db = -1"), (dict(cut_db=math.nan), "cut_db = nan"), (dict(y=y.data_ptr() + 4), "16-byte aligned"),
                     (dict(out=x.data_ptr()), "out overlaps x"), (dict(out=x.data_ptr() + 4 * (S * n - 16)), "out overlaps x"), (dict(out=y.data_ptr() + 64), "y without being y")):
        rc, err = call(**kw)
        assert rc == -1 and "tvc_stream_loudness_f32" in err and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert stage.frames.tolist() == [0, 0] and stage.gain.tolist() == [1.0, 1.0] and float(stage.src_ring.abs().max()) == 0.0
    rc, _ = call()      # and the well-formed call runs (no gain_db, no gains, no shift: all optional)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any()) and stage.frames.tolist() == [2, 2]
    for a, match in (((x, y[:1].contiguous(), None, stage, 0), "a stage for 2 streams"), ((x, y, torch.zeros(S, device=DEV), stage, 0), "shift must be contiguous int32"),
                     ((x, y, None, stage, 1.5), "base must be an integer"), ((x.double(), y, None, stage, 0), "x must be contiguous fp32"),
                     ((x, y, None, _stage(3, block, 2), 0), "a stage for 3 streams")):
        with pytest.raises(ValueError, match=match):
            eng.stream_loudness(*a)
    stage.frames = stage.frames.to(torch.int32)
    with pytest.raises(ValueError, match="stream_loudness: loudness.frames must be contiguous torch.int64"):
        eng.stream_loudness(x, y, None, stage, 0)


# ---- 3. whole streams ----------------------------------------------------------------------------------------------------------------------
GEOM = dict(block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3840)      # a window of 4320: nine whole frames
BASE = 4320 - 480 - 240 - 240 - 480
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
    mic = torch.from_numpy(_signal(S3, 16, 71) * np.float32(2.0)).to(DEV)      # 8 blocks whose level moves every 10 ms
    return tgt, angles, mic


def _stream(gen, tgt, use_graph=False, **stages):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=S3, target=tgt, pitch_shift=[0.0, 2.0, -1.5], device=torch.device(DEV), use_graph=use_graph, **stages, **GEOM)
    st.init_buffer()
    return st


def test_share_zero_is_the_stream_without_the_keyword_and_share_one_is_the_stage_by_hand(gen, model_side):
    tgt, angles, mic = model_side
    eng = gen.engine(torch.device(DEV))
    plain, zero, full = _stream(gen, tgt), _stream(gen, tgt, loudness=_stage(S3, 480, 2, share=0.0)), _stream(gen, tgt, loudness=_stage(S3, 480, 2, share=STREAM_SHARES))
    hand = _stage(S3, 480, 2, share=STREAM_SHARES)
    moved = False
    for i in range(N_BLOCKS):
        blk = mic[:, i * 480:(i + 1) * 480]
        want = plain.audio_callback(blk, noise_angle=angles[i])
        got = zero.audio_callback(blk, noise_angle=angles[i])
        assert _same(got, want) and _same(zero.last_shift, plain.last_shift) and _same(zero.sola_buffer, plain.sola_buffer), f"block {i}: share 0"
        out = full.audio_callback(blk, noise_angle=angles[i])
        # the stage never feeds back: the window, the lag and the SOLA buffer are the plain stream's
        assert _same(full.input_wav, plain.input_wav) and _same(full.last_shift, plain.last_shift) and _same(full.sola_buffer, plain.sola_buffer), f"block {i}"
        assert _same(out, eng.stream_loudness(plain.input_wav, want, plain.last_shift, hand, BASE)), f"block {i}: not the stage applied to the plain block"
        moved |= not _same(out, want)
    assert moved and zero.loudness.frames.tolist() == [2 * N_BLOCKS] * S3 and all(_same(getattr(full.loudness, k), getattr(hand, k)) for k in ("src_ring", "frames", "gain"))


def _run(gen, model_side, use_graph, n_blocks=7):
    tgt, angles, mic = model_side
    stage = _stage(S3, 480, 2, share=STREAM_SHARES)
    st = _stream(gen, tgt, use_graph, loudness=stage)
    outs, keys, graphs = [], [], []
    for i in range(n_blocks):
        if i == 4:
            stage.share.fill_(0.25)
        if i == 5:
            stage.share.copy_(torch.tensor([1.0, 0.0, 0.5]))
            stage.reset([1])
        outs.append(st.audio_callback(mic[:, i * 480:(i + 1) * 480], noise_angle=angles[i]).clone())
        captured = use_graph and st._graph is not None and True in st._graph[1]
        keys.append(st._graph[0] if captured else None)
        graphs.append(st._graph[1][True][0] if captured else None)
    return torch.stack(outs), _state(stage), keys, graphs, st


def test_graph_replay_equals_eager_with_one_capture(gen, model_side):
    """share.fill_ / copy_ and reset([1]) between blocks, and the history advancing: the graph captured at block 2 replays to the end under
    one key and equals eager; a stage at another address or with other params() is another key"""
    eager = _run(gen, model_side, False)
    graph = _run(gen, model_side, True)
    keys, g = graph[2], graph[3]
    assert keys[0] is None and keys[1] is None and keys[2] is not None and all(k == keys[2] for k in keys[2:]), "_graph[0] changed"
    assert all(x is g[2] for x in g[2:]), "a share / a reset captured a new graph"
    assert _same(eager[0], graph[0]), "graph replay is not sample-exact"
    assert all(_same(eager[1][k], graph[1][k]) for k in eager[1]), "the final state differs"
    assert not _same(eager[0][4], eager[0][3]) and eager[1]["frames"].tolist() == [14, 4, 14]      # the share and the reset took effect
    st = graph[4]
    key = st._graph_key()
    assert key == st._graph[0] and any(k[0] == "loudness" for k in key if isinstance(k, tuple) and k and isinstance(k[0], str))
    old = st.loudness
    st.loudness = _stage(S3, 480, 2, share=STREAM_SHARES)      # the same parameters at another address
    assert st._graph_key() != key
    for kw in (dict(smooth=1), dict(floor_db=-50.0), dict(boost_db=6.0), dict(cut_db=20.0)):
        twin = _stage(S3, 480, **dict(dict(smooth=2), **kw))
        if twin.window == old.window:      # the same addresses: only params() tell them apart
            for name in ("share", "src_ring", "out_ring", "frames", "gain", "gain_db"):
                setattr(twin, name, getattr(old, name))
        st.loudness = twin
        assert st._graph_key() != key, f"{kw} did not change the graph key"
    twin = _stage(S3, 480, 2)
    for name in ("share", "src_ring", "out_ring", "frames", "gain", "gain_db"):
        setattr(twin, name, getattr(old, name))
    st.loudness = twin
    assert st._graph_key() == key, "values, not addresses or params(), went into the key"
    st.loudness = _stage(S3, 480, 2)      # a new stage on the same stream: the next block captures anew
    tgt, angles, mic = model_side
    st.audio_callback(mic[:, :480], noise_angle=angles[0])
    assert st._graph[1][True][0] is not g[2]


def test_with_a_gate_and_a_door_the_order_is_sola_loudness_gate_door(gen, model_side):
    from tinyvc_amd.module.infer import StreamDoor, StreamGate
    tgt, angles, mic = model_side
    eng = gen.engine(torch.device(DEV))
    pcm = (torch.from_numpy(_signal(S3, N_BLOCKS * 4, 81) * np.float32(20.0)).clamp(-1, 1) * 32767).to(torch.int16).to(DEV)      # 48 kHz: 960 per block
    gate_kw = dict(threshold_db=-30.0, hold_size=240, attack_size=240, release_size=480, lookahead_size=480, sub_frame=240, device=DEV)
    door_kw = dict(block_size=480, input_gain=-1.0, output_gain=2.0, device=DEV)
    st = _stream(gen, tgt, loudness=_stage(S3, 480, 2, share=STREAM_SHARES), gate=StreamGate(S3, 480, **gate_kw), door=StreamDoor(S3, 48000, **door_kw))
    hand, hand_stage, hand_gate, hand_door = _stream(gen, tgt), _stage(S3, 480, 2, share=STREAM_SHARES), StreamGate(S3, 480, **gate_kw), StreamDoor(S3, 48000, **door_kw)
    hand_door.prepare(eng)
    other = False
    for i in range(N_BLOCKS):
        blk = pcm[:, i * 960:(i + 1) * 960]
        got = st.audio_callback_pcm(blk, noise_angle=angles[i])
        sola = hand.audio_callback(hand_door.push(eng, blk), noise_angle=angles[i])
        level = eng.stream_loudness(hand.input_wav, sola, hand.last_shift, hand_stage, BASE)
        gated = eng.stream_gate(hand.input_wav, level, hand.last_shift, hand_gate, BASE)
        assert got.dtype == torch.int16 and _same(got, hand_door.pull(eng, gated)), f"block {i}"
        other |= not _same(gated, eng.stream_gate(hand.input_wav, sola, hand.last_shift, StreamGate(S3, 480, **gate_kw), BASE))
    assert other, "the stage changed nothing: the test would pass without it"
    assert _same(st.loudness.gain, hand_stage.gain) and _same(st.gate.gain, hand_gate.gain)


# ---- 4. Generator.convert ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["equal", "ragged", "ragged_in_place", "alpha_protect", "auto_pitch"])
def test_convert_with_loudness_is_the_launch_behind_the_plain_call(gen, case, monkeypatch):
    from tinyvc_amd.module.infer import generator
    from tinyvc_amd.module.tinyvc.feature_retrieval import LoudnessMatch
    from tinyvc_amd.module.utils import autopad_waveform
    eng = gen.engine(torch.device(DEV))
    wf = (synth.synth_wave(2, 9500, seed=1) * torch.tensor([[1.0], [0.05]])).to(DEV)      # (9500 is padded to 9600; the second speaker murmurs)
    tgt = synth.synth_index(256, seed=2).to(DEV)
    angle = synth.synth_angle(2, 20, 3).to(DEV)
    kw = dict(equal={}, ragged=dict(lengths=[9500, 7000]), ragged_in_place=dict(lengths=[9500, 7000]), alpha_protect=dict(alpha=[0.2, 0.4], protect=0.5),
              auto_pitch=dict(auto_pitch=180.0, return_shift=True))[case]
    assert not generator.loudness_in_place(2, torch.device(DEV)), "two rows do not fill the device: convert writes a tensor of its own"
    if case == "ragged_in_place":      # the form a batch with a row per compute unit takes
        monkeypatch.setattr(generator, "loudness_in_place", lambda rows, device: True)
    share = _dev([0.8, 1.0]) if case.startswith("ragged") else [0.8, 1.0]      # a device tensor, used in place, or floats
    plain = gen.convert(wf, tgt, 1.0, noise_angle=angle, **kw)
    got = gen.convert(wf, tgt, 1.0, noise_angle=angle, loudness=share, **kw)
    if case == "auto_pitch":
        assert _same(got[1], plain[1])
        plain, got = plain[0], got[0]
    lens = [9600, 7200] if case.startswith("ragged") else None
    want = eng.loudness_match(autopad_waveform(wf), plain, _dev([0.8, 1.0]), lengths=lens)
    assert _same(got, want) and not _same(got, plain), case
    zero = gen.convert(wf, tgt, 1.0, noise_angle=angle, loudness=0.0, **kw)
    assert _same(zero[0] if case == "auto_pitch" else zero, plain), f"{case}: loudness = 0.0 is not the plain call"
    if case == "equal":      # the settings ride on a LoudnessMatch, the share on a device tensor used in place
        t = _dev([0.8, 1.0])
        got = gen.convert(wf, tgt, 1.0, noise_angle=angle, loudness=LoudnessMatch(t, sub_frame=120, smooth=1, boost_db=6.0))
        assert _same(got, eng.loudness_match(autopad_waveform(wf), plain, t, settings=_settings(1, 120, boost_db=6.0)))
        rms = lambda v: float(v.double().pow(2).mean().sqrt())      # (printed, not held: the murmuring speaker's level before and after)
        print(f"rms in {rms(wf[0]):.4f} / {rms(wf[1]):.4f}, plain {rms(plain[0]):.4f} / {rms(plain[1]):.4f}, matched {rms(want[0]):.4f} / {rms(want[1]):.4f}")


@pytest.mark.parametrize("form", ["equal", "ragged", "ragged_in_place"])
def test_convert_with_loudness_is_captured_once_and_replays(gen, form, monkeypatch):
    """convert(..., loudness=device tensor) inside a graph capture - no host synchronisation, no copy from the host -: the replay follows
    another input and another share, read when the kernels run, and equals the eager call on them"""
    from tinyvc_amd.module.infer import generator
    if form == "ragged_in_place":
        monkeypatch.setattr(generator, "loudness_in_place", lambda rows, device: True)
    tgt = synth.synth_index(256, seed=2).to(DEV)
    first = (synth.synth_wave(2, 9600, seed=5) * torch.tensor([[1.0], [0.05]])).to(DEV)
    second = (synth.synth_wave(2, 9600, seed=6) * torch.tensor([[0.1], [0.7]])).to(DEV)
    angle = synth.synth_angle(2, 20, 3).to(DEV)
    kw = {} if form == "equal" else dict(lengths=[9600, 7000])
    share, buf = _dev([0.8, 1.0]), first.clone()
    gen.convert(buf, tgt, 1.0, noise_angle=angle, loudness=share, **kw)      # eager once: weights packed, index prepared, workspace grown
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        wave = gen.convert(buf, tgt, 1.0, noise_angle=angle, loudness=share, **kw)
    buf.copy_(second)
    share.copy_(_dev([0.3, 0.6]))
    g.replay()
    torch.cuda.synchronize()
    want = gen.convert(second, tgt, 1.0, noise_angle=angle, loudness=[0.3, 0.6], **kw)
    assert _same(wave, want), "the replay did not follow the new input and share"
    assert not _same(want, gen.convert(second, tgt, 1.0, noise_angle=angle, loudness=[0.8, 1.0], **kw)) and not _same(want, gen.convert(second, tgt, 1.0, noise_angle=angle, **kw))
