"""The streams' spectral suppressor on the GPU (tvc_stream_denoise_f32, denoise.hip) against the fp64 restatement of its definition
(tests/helpers_denoise.py).

Numerics: the yardstick is the same restatement evaluated in fp32 on the CPU (torch.fft in float32) on the same inputs; the kernel may be
at most 8 x the yardstick's error, per stream and per array - its factorisation (5 x 64 with table twiddles and untangling, against
pocketfft) and summation order differ by a handful of roundings per value, while a wrong twiddle, bin, lane map or overlap offset shows at
1e-3 and up.  Sample errors are normalised by the stream's input peak, smooth / noise errors by the largest fp64 entry of the array (both
sides of the comparison by the same number).  Every case prints a `[denoise]` line with the measured figures (profiles/stream_denoise_edges.txt).

Exact: block cuts, S and neighbours, aliasing, zeros, muted stretches - bit for bit.  Then the behaviour the issue states for the
definition, the library's refusals, and whole streams: latency, the window's contents, graph replay, denoise=None, the entry script."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import helpers_denoise as hd
from helpers import state_dicts
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S5, N = 5, 15360      # 96 frames at hop 160, 48 at hop 320; whole blocks of 160, 320, 480 and 1920
GEOMETRIES = [(160, 160), (480, 160), (1920, 160), (320, 320), (1920, 320)]
RATIO = 8.0
SETTINGS = dict(strength=2.0, smooth_ms=40.0, adapt_s=1.0, clamp=2.0)
MUTE = (4000, 5500)      # stream 4's exact zeros: longer than a frame and a hop


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


@functools.lru_cache(maxsize=None)
def _inputs():
    """[5, N] fp32: zeros; white noise at -50 dBFS; that noise plus 220 Hz / 1760 Hz bursts with edges at arbitrary samples; a +-1 square
    wave; noise that falls to exact zeros for more than 640 samples and returns"""
    rng = np.random.default_rng(11)
    t = np.arange(N)
    noise = rng.standard_normal(N) * 10.0 ** (-50.0 / 20.0)
    x = np.zeros((S5, N))
    x[1] = noise
    on = ((t >= 1234) & (t < 5003)) | ((t >= 9001) & (t < 13777))
    x[2] = noise + on * (0.25 * np.sin(2 * np.pi * 220.0 * t / 24000) + 0.25 * np.sin(2 * np.pi * 1760.0 * t / 24000))
    x[3] = np.where((t // 53) % 2 == 0, 1.0, -1.0)
    x[4] = rng.standard_normal(N) * 10.0 ** (-50.0 / 20.0)
    x[4, MUTE[0]:MUTE[1]] = 0.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _suppressor(S, block, hop, reduction_db=18.0):
    from tinyvc_amd.module.infer import StreamDenoise
    dn = StreamDenoise(S, block, reduction_db=reduction_db, hop=hop, warmup_ms=8 * hop / 24.0, device=DEV, **SETTINGS)
    assert dn.warm == 8 and dn.delay_size == 640 - hop
    return dn


STATE = ("hist", "ola", "smooth", "noise", "frames", "noise_db")


def _state(dn):
    return {k: getattr(dn, k).cpu().clone() for k in STATE}


def _run_gpu(x, block, hop, reduction_db=18.0, alias=False, dn=None, per_block=None):
    """x [S, n] through the kernel in blocks of `block` -> (out [S, n] on the CPU, the state after the last block)"""
    eng = _engine()
    x = torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV)
    S, n = x.shape
    dn = dn if dn is not None else _suppressor(S, block, hop, reduction_db)
    outs = []
    for i in range(0, n, block):
        blk = x[:, i:i + block].contiguous()
        out = eng.stream_denoise(blk, dn, out=blk if alias else None)
        assert not alias or out.data_ptr() == blk.data_ptr()
        outs.append(out.cpu())
        if per_block is not None:
            per_block(i // block, dn)
    return torch.cat(outs, dim=1), _state(dn)


@functools.lru_cache(maxsize=None)
def _restated(hop, reduction_db=18.0):
    """the fp64 reference and the fp32 yardstick over the five streams, computed once per hop (the definition does not depend on the cut)"""
    from tinyvc_amd.module.infer.stream import denoise_constants
    c = denoise_constants(hop, SETTINGS["strength"], SETTINGS["smooth_ms"], SETTINGS["adapt_s"], SETTINGS["clamp"], 8 * hop / 24.0)
    ref = [hd.run_stream(row, N, reduction_db, c, hop) for row in _inputs()]
    yard = [hd.run_stream(row, N, reduction_db, c, hop, dtype=torch.float32) for row in _inputs()]
    return ref, yard


def _hold(got, yard, ref, norm, what):
    """|got - ref| against RATIO x |yard - ref|, both over `norm`; prints the figures first"""
    ref = ref.double()
    e_k = float((torch.as_tensor(got).double() - ref).abs().max()) / norm
    e_y = float((yard.double() - ref).abs().max()) / norm
    print(f"[denoise] {what}: kernel {e_k:.3e}, yardstick {e_y:.3e}" + (f", ratio {e_k / e_y:.2f}" if e_y > 0 else ""))
    assert e_k <= RATIO * e_y, f"{what}: the kernel is {e_k:.3e} off the fp64 definition, the fp32 yardstick {e_y:.3e}"
    return e_k, e_y


# ---- 1. numerics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,hop", GEOMETRIES)
def test_kernel_against_the_fp64_restatement(block, hop):
    x = _inputs()
    out, st = _run_gpu(x, block, hop)
    ref, yard = _restated(hop)
    for s in range(S5):
        (r_out, r), (y_out, y) = ref[s], yard[s]
        peak = float(np.abs(x[s]).max())
        tag = f"block {block} hop {hop} stream {s}"
        if peak == 0.0:
            assert float(out[s].abs().max()) == 0.0 and float(r_out.abs().max()) == 0.0
            continue
        _hold(out[s], y_out, r_out, peak, f"{tag} samples")
        _hold(st["ola"][s], y.ola, r.ola, peak, f"{tag} ola")
        assert _same(st["hist"][s], torch.from_numpy(x[s, N - (640 - hop):].copy())), f"{tag}: hist is not the input's tail"
        for name in ("smooth", "noise"):
            _hold(st[name][s], getattr(y, name), getattr(r, name), float(getattr(r, name).max()), f"{tag} {name}")
        assert int(st["frames"][s]) == r.frames == y.frames, tag
        if r.noise_db() > -150.0:
            assert abs(float(st["noise_db"][s]) - r.noise_db()) <= 1e-3, (tag, float(st["noise_db"][s]), r.noise_db())
    assert [int(f) for f in st["frames"]][:4] == [0] + [N // hop] * 3 and 0 < int(st["frames"][4]) < N // hop


@pytest.mark.parametrize("hop", [160, 320])
def test_reduction_0_is_the_delayed_input(hop):
    x = _inputs()
    out, st = _run_gpu(x, 1920, hop, reduction_db=0.0)
    _, yard = _restated(hop, 0.0)
    D = 640 - hop
    for s in range(1, S5):
        want = torch.cat([torch.zeros(D, dtype=torch.float64), torch.from_numpy(x[s].astype(np.float64))[:-D]])
        _hold(out[s], yard[s][0], want, float(np.abs(x[s]).max()), f"reduction 0, hop {hop} stream {s} samples against the delayed input")
    assert [int(f) for f in st["frames"]][1:4] == [N // hop] * 3 and float(st["noise"][1].max()) > 0, "the state did not advance"


# ---- 2. what must be exact -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _whole(hop):
    """the five streams at block 1920, computed once per hop"""
    return _run_gpu(_inputs(), 1920, hop)


@pytest.mark.parametrize("block,hop", [(160, 160), (480, 160), (320, 320), (960, 320)])
def test_the_cut_into_blocks_changes_no_bit(block, hop):
    out, st = _run_gpu(_inputs(), block, hop)
    want, want_st = _whole(hop)
    assert _same(out, want)
    assert all(_same(st[k], want_st[k]) for k in STATE), [k for k in STATE if not _same(st[k], want_st[k])]


@pytest.mark.parametrize("hop", [160, 320])
def test_a_stream_alone_equals_its_row_among_five(hop):
    want, want_st = _whole(hop)
    for s in range(S5):
        out, st = _run_gpu(_inputs()[s:s + 1], 1920, hop)
        assert _same(out[0], want[s]), s
        assert all(_same(st[k][0], want_st[k][s]) for k in STATE), s
    # and with other neighbours: the rows in another order
    order = [3, 0, 4, 2, 1]
    out, st = _run_gpu(_inputs()[order], 1920, hop)
    assert _same(out, want[order]) and all(_same(st[k], want_st[k][order]) for k in STATE)


def test_zeros_emit_zeros_and_a_muted_stretch_moves_no_estimate():
    hop = 160
    x = _inputs()
    snaps = []
    out, st = _run_gpu(x, hop, hop, per_block=lambda i, dn: snaps.append((dn.smooth[4].cpu().clone(), dn.noise[4].cpu().clone(), int(dn.frames[4]))))
    assert _same(out[0], torch.zeros(N)) and int(st["frames"][0]) == 0
    assert all(_same(st[k][0], torch.zeros_like(st[k][0])) for k in ("hist", "ola", "smooth", "noise")) and abs(float(st["noise_db"][0]) + 200.0) <= 1e-3
    # frame m of the stream covers input samples (m + 1) hop - 640 .. (m + 1) hop
    muted = [m for m in range(1, N // hop) if MUTE[0] <= (m + 1) * hop - 640 and (m + 1) * hop <= MUTE[1]]
    assert len(muted) >= 3
    for m in range(1, N // hop):
        moved = not (_same(snaps[m][0], snaps[m - 1][0]) and _same(snaps[m][1], snaps[m - 1][1]))
        assert moved == (m not in muted) and snaps[m][2] - snaps[m - 1][2] == (0 if m in muted else 1), m
    # the samples under the muted frames alone are zeros
    # output sample j is made of frames ceil((j - 639) / hop) .. j // hop: where all of them are muted it is zero, and nowhere else nearby
    a, b = (muted[0] + 3) * hop, (muted[-1] + 1) * hop
    assert a < b and _same(out[4, a:b], torch.zeros(b - a)) and float(out[4, a - hop:a].abs().max()) > 0 and float(out[4, b:b + hop].abs().max()) > 0


@pytest.mark.parametrize("block,hop", [(480, 160), (1920, 160), (1920, 320)])
def test_out_may_be_the_input(block, hop):
    out, st = _run_gpu(_inputs(), block, hop, alias=True)
    want, want_st = _whole(hop)
    assert _same(out, want) and all(_same(st[k], want_st[k]) for k in STATE)


def test_the_reduction_is_read_when_the_kernel_runs():
    hop, block = 160, 1920
    x = _inputs()[1:3]
    dn = _suppressor(2, block, hop, 18.0)

    def move(i, d):
        if i == 3:
            d.reduction_db.fill_(6.0)
        if i == 5:
            d.reduction_db.copy_(torch.tensor([0.0, 30.0]))
    out, _ = _run_gpu(x, block, hop, dn=dn, per_block=move)
    from tinyvc_amd.module.infer.stream import denoise_constants
    c = denoise_constants(hop, SETTINGS["strength"], SETTINGS["smooth_ms"], SETTINGS["adapt_s"], SETTINGS["clamp"], 8 * hop / 24.0)
    for s in range(2):
        r = hd.Restated(hop, *c)
        y = hd.Restated(hop, *c, dtype=torch.float32)
        red = lambda i: 18.0 if i <= 3 else 6.0 if i <= 5 else (0.0, 30.0)[s]      # a change after block i takes effect at block i + 1
        want = torch.cat([r.run(x[s, i * block:(i + 1) * block], red(i)) for i in range(N // block)])
        yard = torch.cat([y.run(x[s, i * block:(i + 1) * block], red(i)) for i in range(N // block)])
        _hold(out[s], yard, want, float(np.abs(x[s]).max()), f"live reduction, stream {s} samples")
    steady = _whole(hop)[0][1:3]
    assert _same(out[:, :4 * block], steady[:, :4 * block]) and not _same(out[:, 4 * block:5 * block], steady[:, 4 * block:5 * block])


# ---- 3. behaviour ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [160, 320])
def test_the_kernel_behaves_as_the_issue_states(hop):
    from tinyvc_amd.module.infer import StreamDenoise
    x = hd.behaviour_input()
    b = hd.BEHAVIOUR
    dn = StreamDenoise(1, 9600, reduction_db=b["reduction_db"], hop=hop, strength=b["strength"], smooth_ms=b["smooth_ms"], adapt_s=b["adapt_s"],
                       clamp=b["clamp"], warmup_ms=b["warmup_ms"], device=DEV)
    out, _ = _run_gpu(x[None], 9600, hop, dn=dn)
    hd.check_behaviour(x, out[0].numpy(), 640 - hop)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_header_says():
    eng = _engine()
    S, block = 2, 480
    x = torch.ones(S, block, device=DEV)
    out = torch.full((S, block), 7.0, device=DEV)
    dn = _suppressor(S, block, 160)
    good = dict(x=x.data_ptr(), out=out.data_ptr(), S=S, block=block, hop=160, a_s=0.5, a_n=0.9, clamp=2.0, beta=2.0, warm=8, reduction_db=dn.reduction_db.data_ptr(),
                hist=dn.hist.data_ptr(), ola=dn.ola.data_ptr(), smooth=dn.smooth.data_ptr(), noise=dn.noise.data_ptr(), frames=dn.frames.data_ptr(), noise_db=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        p = lambda v: ctypes.c_void_p(v) if v is not None else None
        rc = eng.lib.tvc_stream_denoise_f32(eng.ctx, eng._stream(), p(a["x"]), p(a["out"]), a["S"], a["block"], a["hop"], a["a_s"], a["a_n"], a["clamp"], a["beta"],
                                            a["warm"], p(a["reduction_db"]), p(a["hist"]), p(a["ola"]), p(a["smooth"]), p(a["noise"]), p(a["frames"]),
                                            p(a["noise_db"]))
        return rc, eng.lib.tvc_last_error(eng.ctx).decode()

    for kw, text in ((dict(hop=128), "hop = 128 is neither 160 nor 320"), (dict(hop=320), "block = 480 is not a whole number of 320-sample hops"),
                     (dict(block=0), "block = 0 is shorter than one hop"), (dict(block=4097 * 160), "block / hop = 4097 frames is above 4096"),
                     (dict(x=None), "NULL pointer"), (dict(out=None), "NULL pointer"), (dict(reduction_db=None), "NULL pointer"), (dict(hist=None), "NULL pointer"),
                     (dict(ola=None), "NULL pointer"), (dict(smooth=None), "NULL pointer"), (dict(noise=None), "NULL pointer"), (dict(frames=None), "NULL pointer"),
                     (dict(S=0), "S <= 0"), (dict(a_s=1.0), "outside [0, 1)"), (dict(a_s=-0.1), "outside [0, 1)"), (dict(a_n=1.0), "outside [0, 1)"),
                     (dict(a_n=-1e-3), "outside [0, 1)"), (dict(clamp=0.99), "clamp = 0.99 is below 1"), (dict(beta=-0.5), "beta = -0.5 is negative"),
                     (dict(warm=-1), "warm = -1 is negative"), (dict(a_s=math.nan), "not all finite"), (dict(a_n=math.inf), "not all finite"),
                     (dict(clamp=math.inf), "not all finite"), (dict(beta=math.nan), "not all finite")):
        rc, err = call(**kw)
        assert rc == -1 and "tvc_stream_denoise_f32" in err and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert dn.frames.tolist() == [0, 0] and float(dn.smooth.abs().max()) == 0.0 and float(dn.hist.abs().max()) == 0.0
    rc, _ = call()      # and the well-formed call runs (no noise_db: it is optional)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any()) and dn.frames.tolist() == [3, 3] and float(dn.noise_db[0]) == -200.0      # (not written: the class's initial value)
    # the checked wrapper refuses shapes, dtypes and foreign suppressors before the library is called
    for a, match in (((x[:1].contiguous(), dn), "a suppressor for 2 streams"), ((x.double(), dn), "blocks must be contiguous fp32"),
                     ((x, _suppressor(3, block, 160)), "a suppressor for 3 streams"), ((x, dn, out[:, :100]), "out must be contiguous fp32")):
        with pytest.raises(ValueError, match=match):
            eng.stream_denoise(*a)
    twin = _suppressor(S, block, 160)
    twin.frames = twin.frames.to(torch.int64)
    with pytest.raises(ValueError, match="denoise.frames must be contiguous torch.int32"):
        eng.stream_denoise(x, twin)


# ---- 5. whole streams --------------------------------------------------------------------------------------------------------------------------
S2, BLOCK, N_BLOCKS = 2, 1920, 8      # the default window: 13 440 samples, 28 frames


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
    angles = [synth.synth_angle(S2, 28, 700 + i).to(DEV) for i in range(N_BLOCKS)]
    mic = torch.from_numpy(np.array(_inputs()[[2, 4], :N_BLOCKS * BLOCK])).to(DEV)
    return tgt, angles, mic


def _stream(gen, tgt, use_graph=False, **kw):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=S2, target=tgt, pitch_shift=[0.0, 2.0], device=torch.device(DEV), use_graph=use_graph, **kw)
    st.init_buffer()
    return st


def test_the_window_holds_the_suppressed_block_and_the_latency_grows(gen, model_side):
    tgt, angles, mic = model_side
    eng = gen.engine(torch.device(DEV))
    plain = _stream(gen, tgt)
    for hop in (160, 320):
        dn = _suppressor(S2, BLOCK, hop)
        st = _stream(gen, tgt, denoise=dn)
        assert st.latency_samples == tuple(v + dn.delay_size for v in plain.latency_samples) and dn.delay_size == 640 - hop
        assert st.latency_seconds == tuple(v / 24000 for v in st.latency_samples)
        hand = _suppressor(S2, BLOCK, hop)
        for i in range(3):
            blk = mic[:, i * BLOCK:(i + 1) * BLOCK].contiguous()
            out = st.audio_callback(blk, noise_angle=angles[i])
            want = eng.stream_denoise(blk, hand)
            assert _same(st.input_wav[:, -BLOCK:], want) and not _same(want, blk), (hop, i)
            assert all(_same(getattr(dn, k), getattr(hand, k)) for k in STATE)
        assert out.shape == (S2, BLOCK) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 1e-3


def test_denoise_none_is_the_stream_as_it_was(gen, model_side):
    tgt, angles, mic = model_side
    a, b = _stream(gen, tgt), _stream(gen, tgt, denoise=None)
    for i in range(3):
        blk = mic[:, i * BLOCK:(i + 1) * BLOCK]
        assert _same(a.audio_callback(blk, noise_angle=angles[i]), b.audio_callback(blk, noise_angle=angles[i])), i
        assert _same(a.input_wav, b.input_wav) and _same(a.last_shift, b.last_shift)
    assert a._graph_key() == b._graph_key()


def _run(gen, model_side, use_graph):
    tgt, angles, mic = model_side
    dn = _suppressor(S2, BLOCK, 160)
    st = _stream(gen, tgt, use_graph, denoise=dn)
    outs, graphs = [], []
    for i in range(N_BLOCKS):
        if i == 4:
            dn.reduction_db.fill_(6.0)
        if i == 6:
            dn.reset([1])
        outs.append(st.audio_callback(mic[:, i * BLOCK:(i + 1) * BLOCK], noise_angle=angles[i]).clone())
        graphs.append(st._graph[1][True][0] if use_graph and st._graph is not None and True in st._graph[1] else None)
    return torch.stack(outs), _state(dn), graphs, st, st.input_wav.clone()


def test_graph_replay_equals_eager_with_one_capture(gen, model_side):
    """reduction_db.fill_ and denoise.reset([1]) between blocks: the graph captured at block 2 replays to the end (the same graph object)
    and equals eager; a suppressor at another address or with other params() is another key."""
    eager = _run(gen, model_side, False)
    graph = _run(gen, model_side, True)
    g = graph[2]
    assert g[0] is None and g[1] is None and g[2] is not None and all(x is g[2] for x in g[2:]), "a reduction / a reset captured a new graph"
    assert len(g[2:]) >= 5
    assert _same(eager[0], graph[0]), "graph replay is not sample-exact"
    assert all(_same(eager[1][k], graph[1][k]) for k in STATE) and _same(eager[4], graph[4]), "the final state differs"
    assert eager[1]["frames"].tolist() == [N_BLOCKS * BLOCK // 160, 2 * BLOCK // 160], "reset([1]) did not restart stream 1's count"
    st = graph[3]
    key = st._graph_key()
    assert key == st._graph[0]
    old = st.denoise
    st.denoise = _suppressor(S2, BLOCK, 160)      # the same parameters at another address
    assert st._graph_key() != key
    from tinyvc_amd.module.infer import StreamDenoise
    base = dict(reduction_db=18.0, hop=160, warmup_ms=8 * 160 / 24.0, device=DEV, **SETTINGS)
    for kw in (dict(strength=1.5), dict(smooth_ms=20.0), dict(adapt_s=0.5), dict(clamp=3.0), dict(warmup_ms=100.0)):
        args = dict(base)
        args.update(kw)
        twin = StreamDenoise(S2, BLOCK, **args)
        for name in ("reduction_db",) + STATE:      # the same addresses: only params() tell them apart
            setattr(twin, name, getattr(old, name))
        st.denoise = twin
        assert st._graph_key() != key, f"{kw} did not change the graph key"
    twin = _suppressor(S2, BLOCK, 160, reduction_db=3.0)
    for name in ("reduction_db",) + STATE:
        setattr(twin, name, getattr(old, name))
    st.denoise = twin
    assert st._graph_key() == key, "values, not addresses or params(), went into the key"


E2E_BLOCKS = 6


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise")
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(500, seed=2), d / "index.pt")
    mic = torch.from_numpy(_inputs()[2, :E2E_BLOCKS * 1920].copy())
    audio_io.save(str(d / "mic.wav"), mic[None], 24000)
    common = ["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "index.pt"), "--input-wav", str(d / "mic.wav"), "--streams", "2",
              "-d", DEV]
    return d, common


def test_infer_streaming_denoise_runs_and_prints_the_estimate(files, capsys):
    import infer_streaming
    d, common = files
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--denoise", "12", "--output-wav", str(d / "clean.wav")]) == 0
    text = capsys.readouterr().out
    assert "Noise suppressor: up to 12 dB per bin (strength 2, smoothing 40 ms, adaptation 1 s, warm-up 200 ms) in 640-sample frames at a hop of 160: 20.0 ms of delay" in text
    assert "Latency 260.0 to 340.0 ms" in text and "+ the suppressor's 480 samples" in text
    lines = [l for l in text.splitlines() if "noise estimate" in l]
    assert len(lines) == 2 and lines[0].startswith("stream 0: noise estimate ") and lines[0].endswith(" dB re full scale")
    db = float(lines[0].split("noise estimate ")[1].split(" dB")[0])
    assert -150.0 < db < 0.0, db      # an estimate exists (the empty one reads -200) and lies below full scale
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--output-wav", str(d / "plain.wav")]) == 0
    text = capsys.readouterr().out
    assert "Noise suppressor" not in text and "noise estimate" not in text and "Latency 240.0 to 320.0 ms" in text
    assert open(d / "plain.wav", "rb").read() != open(d / "clean.wav", "rb").read()
