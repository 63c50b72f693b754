"""The streams' spectral suppressor without a GPU: the geometry entry (tvc_stream_denoise_geometry: no context, no device) and its messages,
StreamDenoise's and the stream constructors' refusals, infer_streaming.py's --denoise flags, and the fp64 restatement of the definition
(tests/helpers_denoise.py) held against properties of the definition itself: reduction 0 is the delayed input, a stream cut into blocks is
the whole, and the behaviour the issue states for it."""
import ctypes
import inspect
import math
import types

import numpy as np
import pytest
import torch

import helpers_denoise as hd
from tinyvc_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, block, hop):
    frames, delay = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.tvc_stream_denoise_geometry(block, hop, ctypes.byref(frames), ctypes.byref(delay))
    return rc, frames.value, delay.value, lib.tvc_stream_denoise_geometry_message(block, hop).decode()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_rule_and_messages(lib):
    assert _geometry(lib, 160, 160) == (0, 1, 480, "")
    assert _geometry(lib, 480, 160) == (0, 3, 480, "")
    assert _geometry(lib, 1920, 160) == (0, 12, 480, "")
    assert _geometry(lib, 1920, 320) == (0, 6, 320, "")
    assert _geometry(lib, 4096 * 160, 160) == (0, 4096, 480, "")      # the last that fits
    assert lib.tvc_stream_denoise_geometry(1920, 160, None, None) == 0      # the out pointers are optional
    for args, why in (((480, 320), "block = 480 is not a whole number of 320-sample hops"),
                      ((1920, 128), "hop = 128 is neither 160 nor 320"),
                      ((1920, 0), "hop = 0 is neither 160 nor 320"),
                      ((0, 160), "block = 0 is shorter than one hop of 160 samples"),
                      ((-160, 160), "block = -160 is shorter than one hop of 160 samples"),
                      ((4097 * 160, 160), "block / hop = 4097 frames is above 4096"),
                      ((4097 * 320, 320), "block / hop = 4097 frames is above 4096")):
        rc, frames, delay, msg = _geometry(lib, *args)
        assert (rc, frames, delay) == (-1, -7, -7) and msg == why, (args, msg)
    # the call itself wants a context before anything else
    assert lib.tvc_stream_denoise_f32(None, None, None, None, 1, 1920, 160, 0.5, 0.5, 2.0, 2.0, 8, None, None, None, None, None, None, None) == -1


def test_engine_wrapper_of_the_rule(lib):
    from tinyvc_amd import engine
    assert engine.stream_denoise_geometry(1920, 160, lib) == (12, 480)
    assert engine.stream_denoise_geometry(1920, lib=lib) == (12, 480)
    assert engine.stream_denoise_geometry(1920, 320, lib) == (6, 320)
    with pytest.raises(ValueError, match="stream denoise geometry: hop = 128 is neither 160 nor 320"):
        engine.stream_denoise_geometry(1920, 128, lib=lib)
    with pytest.raises(ValueError, match="hop must be an integer"):
        engine.stream_denoise_geometry(1920, 160.0, lib=lib)
    with pytest.raises(ValueError, match="block must be an integer"):
        engine.stream_denoise_geometry(True, 160, lib=lib)
    assert list(inspect.signature(engine.Engine.stream_denoise).parameters)[1:] == ["blocks", "denoise", "out"]


# ---- StreamDenoise -----------------------------------------------------------------------------------------------------------------------
def test_stream_denoise_refuses_before_allocating(lib, monkeypatch):
    from tinyvc_amd.module.infer import StreamDenoise
    from tinyvc_amd.module.infer import stream as stream_mod

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    for name in ("zeros", "ones", "full", "tensor", "empty"):
        monkeypatch.setattr(stream_mod.torch, name, no_alloc)
    for device in ("cuda", "cpu"):
        for kw, match in ((dict(n_streams=0), "n_streams"), (dict(block_size=1920.0), "block_size"), (dict(hop=True), "hop"),
                          (dict(hop=128), "StreamDenoise: stream denoise geometry: hop = 128 is neither 160 nor 320"),
                          (dict(block_size=480, hop=320), "block = 480 is not a whole number of 320-sample hops"),
                          (dict(block_size=4097 * 160), "block / hop = 4097 frames is above 4096"),
                          (dict(reduction_db=float("nan")), "reduction_db"), (dict(reduction_db="12"), "reduction_db"),
                          (dict(reduction_db=[12.0, 6.0]), r"one per stream \(3\)"), (dict(strength=-1.0), "strength"), (dict(strength=float("inf")), "strength"),
                          (dict(strength=1e39), "not a finite fp32 number"), (dict(smooth_ms=-1.0), "smooth_ms"), (dict(smooth_ms=float("nan")), "smooth_ms"),
                          (dict(smooth_ms=1e12), "its fp32 coefficient is 1"), (dict(adapt_s=-0.5), "adapt_s"), (dict(adapt_s=1e9), "its fp32 coefficient is 1"),
                          (dict(clamp=0.5), "clamp must be a finite number >= 1"), (dict(clamp=True), "clamp"), (dict(warmup_ms=-1.0), "warmup_ms"),
                          (dict(warmup_ms=1e12), "more than 2\\^30 frames")):
            args = dict(n_streams=3, block_size=1920, device=device)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                StreamDenoise(**args)
        # a well-formed suppressor on the CPU - or on a GPU that is not there - is refused too, still without allocating
        if device == "cpu" or not torch.cuda.is_available():
            for kw in (dict(), dict(reduction_db=0.0, hop=320), dict(reduction_db=[12.0, 6.0, math.inf], smooth_ms=0.0, adapt_s=0.0, warmup_ms=0.0)):
                with pytest.raises(ValueError, match="live on the GPU"):
                    StreamDenoise(3, 1920, device=device, **kw)
    sig = inspect.signature(StreamDenoise.__init__).parameters
    assert list(sig)[1:] == ["n_streams", "block_size", "reduction_db", "hop", "strength", "smooth_ms", "adapt_s", "clamp", "warmup_ms", "device"]
    assert [sig[k].default for k in list(sig)[3:]] == [12.0, 160, 2.0, 40.0, 1.0, 2.0, 200.0, None]
    assert "guesses" in StreamDenoise.__doc__ and hasattr(StreamDenoise, "reset") and hasattr(StreamDenoise, "params")
    import tinyvc_amd.module.infer as infer_mod
    assert "StreamDenoise" in infer_mod.__all__


def test_the_constants_are_rounded_to_fp32_once(lib):
    from tinyvc_amd.module.infer.stream import denoise_constants
    a_s, a_n, clamp, beta, warm = denoise_constants(160, 2.0, 40.0, 1.0, 2.0, 200.0)
    assert a_s == float(np.float32(math.exp(-160 / (24000 * 0.040)))) and a_n == float(np.float32(math.exp(-160 / 24000.0)))
    assert (clamp, beta, warm) == (2.0, 2.0, 30)
    assert denoise_constants(320, 1.3, 40.0, 1.0, 2.0, 200.0)[3:] == (float(np.float32(1.3)), 15)
    assert denoise_constants(160, 0.0, 0.0, 0.0, 1.0, 0.0) == (0.0, 0.0, 1.0, 0.0, 0)
    assert denoise_constants(160, 2.0, 40.0, 1.0, 2.0, 8 * 160 / 24.0)[4] == 8


# ---- the stream classes ------------------------------------------------------------------------------------------------------------------
def _gen():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def _fake(n_streams, block_size, delay_size=480):
    """what the stream classes look at before any device work"""
    resets = []
    return types.SimpleNamespace(n_streams=n_streams, block_size=block_size, delay_size=delay_size, reset=lambda: resets.append(1), resets=resets)


def test_stream_classes_take_a_suppressor_and_refuse_a_foreign_one(lib):
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    cpu = torch.device("cpu")
    for cls in (BatchedStreamInfer, StreamInfer):
        p = inspect.signature(cls.__init__).parameters
        assert "denoise" in p and p["denoise"].default is None
    plain = BatchedStreamInfer(_gen(), 2, device=cpu)
    assert plain.denoise is None and plain.latency_samples == (5760, 7680)
    with pytest.raises(ValueError, match="denoise: built for 3 streams of 1920-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(_gen(), 2, device=cpu, denoise=_fake(3, 1920))
    with pytest.raises(ValueError, match="denoise: built for 2 streams of 960-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(_gen(), 2, device=cpu, denoise=_fake(2, 960))
    with pytest.raises(ValueError, match="denoise: built for 2 streams"):
        StreamInfer(_gen(), denoise=_fake(2, 1920))
    d = _fake(2, 1920, 320)
    st = BatchedStreamInfer(_gen(), 2, device=cpu, denoise=d)
    assert st.denoise is d and "denoise" in st._graph_key.__doc__
    # the latency grows by the suppressor's delay: 13.3 ms at hop 320, 20 ms at hop 160
    assert st.latency_samples == (5760 + 320, 7680 + 320)
    assert st.latency_seconds == ((5760 + 320) / 24000, (7680 + 320) / 24000)
    st.init_buffer()
    assert d.resets == [1]
    st.denoise = _fake(3, 1920)      # attributes are plain: a foreign suppressor put in later is met at the next init_buffer
    with pytest.raises(ValueError, match="denoise: built for 3 streams"):
        st.init_buffer()


# ---- infer_streaming.py --denoise ----------------------------------------------------------------------------------------------------------
def _args(*argv):
    import infer_streaming
    return infer_streaming, infer_streaming.build_parser().parse_args(list(argv))


def test_cli_denoise_flags(lib):
    m, args = _args()
    assert args.denoise is None and m.check_denoise(args) is None      # absent: today's path
    m, args = _args("--denoise", "12")
    assert m.check_denoise(args) == dict(reduction_db=12.0, hop=160, strength=2.0, adapt_s=1.0, smooth_ms=40.0, warmup_ms=200.0)
    m, args = _args("--denoise", "0", "--denoise-hop", "320", "--denoise-strength", "1.5", "--denoise-adapt", "0.5", "--denoise-smooth", "20",
                    "--denoise-warmup", "0")
    assert m.check_denoise(args) == dict(reduction_db=0.0, hop=320, strength=1.5, adapt_s=0.5, smooth_ms=20.0, warmup_ms=0.0)
    # the model's block, not -c, is what must be whole hops
    m, args = _args("--denoise", "12", "--resample", "-sr", "48000", "-c", "3840")
    assert m.check_denoise(args, m.check_resample(args))["hop"] == 160
    for argv, text in ((("--denoise-hop", "320"), "--denoise-hop without --denoise DB"),
                       (("--denoise-strength", "1", "--denoise-warmup", "10"), "--denoise-strength --denoise-warmup without --denoise DB"),
                       (("--denoise", "nan"), "--denoise: a reduction in dB"),
                       (("--denoise", "12", "--denoise-strength", "-1"), "--denoise-strength -1.0"),
                       (("--denoise", "12", "--denoise-adapt", "inf"), "--denoise-adapt inf"),
                       (("--denoise", "12", "--denoise-smooth", "-3"), "--denoise-smooth -3.0"),
                       (("--denoise", "12", "--denoise-warmup", "nan"), "--denoise-warmup nan"),
                       (("--denoise", "12", "--denoise-adapt", "1e9"), "its fp32 coefficient is 1"),
                       (("--denoise", "12", "-c", "2000"), "block = 2000 is not a whole number of 160-sample hops"),
                       (("--denoise", "12", "-c", "480", "--denoise-hop", "320"), "block = 480 is not a whole number of 320-sample hops")):
        m, args = _args(*argv)
        with pytest.raises(SystemExit) as e:
            m.check_denoise(args)
        assert text in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit):      # argparse holds the hop to its two values
        _args("--denoise", "12", "--denoise-hop", "128")
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--denoise", "12", "-c", "2000", "-encp", "/nonexistent/encoder.pt"])
    assert "not a whole number of 160-sample hops" in str(e.value)
    text = m.build_parser().format_help()
    assert all(f in text for f in ("--denoise DB", "--denoise-hop", "--denoise-strength", "--denoise-adapt", "--denoise-smooth", "--denoise-warmup"))
    assert "guesses" in text


# ---- the restatement against the definition's own properties -------------------------------------------------------------------------------
def _constants(hop, warmup_ms=None, **kw):
    from tinyvc_amd.module.infer.stream import denoise_constants
    s = dict(hd.BEHAVIOUR)
    s.update(kw)
    return denoise_constants(hop, s["strength"], s["smooth_ms"], s["adapt_s"], s["clamp"], s["warmup_ms"] if warmup_ms is None else warmup_ms)


def _signal(n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = rng.standard_normal(n) * 3e-3 + 0.25 * np.sin(2 * np.pi * 220.0 * t / 24000) * ((t > 1234) & (t < 5003))
    x[7000:8700] = 0.0      # a muted stretch longer than a frame and a hop
    return x.astype(np.float32)


@pytest.mark.parametrize("hop", [160, 320])
def test_restatement_with_reduction_0_is_the_delayed_input(lib, hop):
    x = _signal(9600)
    y, r = hd.run_stream(x, 1920, 0.0, _constants(hop), hop)
    D = 640 - hop
    want = torch.cat([torch.zeros(D, dtype=torch.float64), torch.from_numpy(x.astype(np.float64))[:-D]])
    err = float((y - want).abs().max())
    assert err <= 1e-12, err
    assert r.frames > 0 and float(r.noise.max()) > 0, "the state did not advance"


@pytest.mark.parametrize("hop", [160, 320])
def test_restatement_cut_into_blocks_is_the_whole(lib, hop):
    x = _signal(9600)
    c = _constants(hop, warmup_ms=8 * hop / 24.0)
    assert c[4] == 8
    whole, r0 = hd.run_stream(x, 9600, 18.0, c, hop)
    for block in {hop, 3 * hop, 1920}:
        cut, r = hd.run_stream(x, block, 18.0, c, hop)
        assert torch.equal(cut, whole), block
        assert all(torch.equal(getattr(r, k), getattr(r0, k)) for k in ("hist", "ola", "smooth", "noise")) and r.frames == r0.frames
    # the muted stretch holds all-zero frames: they were not counted
    assert r0.frames < 9600 // hop
    # and zeros in, zeros out, nothing moves
    z, rz = hd.run_stream(np.zeros(1920, dtype=np.float32), 1920, 18.0, c, hop)
    assert float(z.abs().max()) == 0.0 and rz.frames == 0 and float(rz.smooth.abs().max()) == 0.0 and rz.noise_db() == -200.0


@pytest.mark.parametrize("hop", [160, 320])
def test_restatement_behaves_as_the_issue_states(lib, hop):
    x = hd.behaviour_input()
    y, _ = hd.run_stream(x, len(x), hd.BEHAVIOUR["reduction_db"], _constants(hop), hop)
    hd.check_behaviour(x, y.numpy(), 640 - hop)
