"""The streaming door without a GPU: the geometry entry (tvc_stream_resample_geometry: no context, no device), StreamDoor's argument checks
and infer_streaming.py --resample's.  Everything is refused on the host, before any device work."""
import ctypes
import math

import pytest
import torch

from tinyvc_amd import _lib
from tinyvc_amd.engine import STREAM_RESAMPLE_LDS_FLOATS, stream_resample_geometry

# in, out, orig, new, width, taps, G, hist, delay, the client block that goes with 1920 samples at 24 kHz
TABLE = [
    (48000, 24000, 2, 1, 13, 28, 7, 27, 7, 3840),
    (44100, 24000, 147, 80, 12, 171, 1, 159, 80, 3528),
    (32000, 24000, 4, 3, 9, 22, 3, 21, 9, 2560),
    (22050, 24000, 147, 160, 7, 161, 1, 154, 160, 1764),
    (16000, 24000, 2, 3, 7, 16, 4, 15, 12, 1280),
    (8000, 24000, 1, 3, 7, 15, 7, 14, 21, 640),
    (24000, 48000, 1, 2, 7, 15, 7, 14, 14, 3840),
    (24000, 44100, 80, 147, 7, 94, 1, 87, 147, 3528),
    (24000, 16000, 3, 2, 10, 23, 4, 22, 8, 1280),
    (24000, 8000, 3, 1, 19, 41, 7, 40, 7, 640),
]


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, in_freq, out_freq, n_in):
    n_out, hist, delay = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.tvc_stream_resample_geometry(in_freq, out_freq, n_in, ctypes.byref(n_out), ctypes.byref(hist), ctypes.byref(delay))
    return rc, n_out.value, hist.value, delay.value


@pytest.mark.parametrize("row", TABLE, ids=[f"{r[0]}-{r[1]}" for r in TABLE])
def test_geometry_reproduces_the_table(lib, row):
    in_freq, out_freq, orig, new, width, taps, G, hist, delay, client = row
    # the table's own columns hang together as the definitions say (and as tinyvc_amd/resample.py computes width)
    g = math.gcd(in_freq, out_freq)
    assert (orig, new) == (in_freq // g, out_freq // g) and width == math.ceil(6 * orig / (min(orig, new) * 0.99)) and taps == 2 * width + orig
    assert G == -(-width // orig) and hist == G * orig + width and delay == G * new
    # the 1920-sample model block and its client block
    n_in, n_out = (client, 1920) if out_freq == 24000 else (1920, client)
    assert _geometry(lib, in_freq, out_freq, n_in) == (0, n_out, hist, delay)
    # a second block size: one group, and 5 groups
    assert _geometry(lib, in_freq, out_freq, orig) == (0, new, hist, delay)
    assert _geometry(lib, in_freq, out_freq, 5 * orig) == (0, 5 * new, hist, delay)
    assert stream_resample_geometry(in_freq, out_freq, n_in, lib) == (n_out, hist, delay)


def test_geometry_refusals(lib):
    assert _geometry(lib, 44100, 24000, 1920)[0] == -1 and _geometry(lib, 48000, 24000, 3839)[0] == -1      # not whole groups
    for bad in ((0, 24000, 10), (24000, 0, 10), (-48000, 24000, 10), (48000, -1, 10), (48000, 24000, 0), (48000, 24000, -2)):
        assert _geometry(lib, *bad)[0] == -1, bad
    assert lib.tvc_stream_resample_geometry(48000, 24000, 3840, None, None, None) == -1
    # the LDS budget: history + block in 16384 floats.  48000 -> 24000 carries 27, so 16356 samples is the last block that fits
    assert STREAM_RESAMPLE_LDS_FLOATS == 16384
    assert _geometry(lib, 48000, 24000, 16356) == (0, 8178, 27, 7) and _geometry(lib, 48000, 24000, 16358)[0] == -1
    assert _geometry(lib, 44100, 24000, 147 * 110) == (0, 80 * 110, 159, 80) and _geometry(lib, 44100, 24000, 147 * 111)[0] == -1
    with pytest.raises(ValueError, match="LDS budget of 16384 floats"):
        stream_resample_geometry(48000, 24000, 16358, lib)
    with pytest.raises(ValueError, match="whole 147-sample groups"):
        stream_resample_geometry(44100, 24000, 1920, lib)
    with pytest.raises(ValueError, match="must be positive"):
        stream_resample_geometry(44100, 24000, 0, lib)
    # a refused call without a context where one is needed
    assert lib.tvc_stream_resample(None, None, None, 0, None, 0, None, 1, 2, 48000, 24000, 0.0) == -1
    assert lib.tvc_stream_resample_prepare(None, 48000, 24000) == -1


def test_equal_rates_have_no_history(lib):
    assert _geometry(lib, 24000, 24000, 1920) == (0, 1920, 0, 0) and _geometry(lib, 44100, 44100, 7) == (0, 7, 0, 0)
    assert _geometry(lib, 24000, 24000, 1 << 20) == (0, 1 << 20, 0, 0)      # nothing is staged: no budget to fit
    assert _geometry(lib, 24000, 24000, 0)[0] == -1


# ---- StreamDoor --------------------------------------------------------------------------------------------------------------------------
def test_stream_door_refuses_before_allocating(lib, monkeypatch):
    from tinyvc_amd.module.infer import StreamDoor
    from tinyvc_amd.module.infer import stream as stream_mod

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    monkeypatch.setattr(stream_mod.torch, "zeros", no_alloc)
    for device in ("cuda", "cpu"):
        with pytest.raises(ValueError, match=r"block_size = 1000 .* 44100 Hz in / 44100 Hz out \(multiples of 80\).*: 960 or 1040"):
            StreamDoor(3, 44100, block_size=1000, device=device)
        with pytest.raises(ValueError, match=r"48000 Hz in / 22050 Hz out \(multiples of 160\).*: 960 or 1120"):
            StreamDoor(3, 48000, 22050, block_size=1000, device=device)
        with pytest.raises(ValueError, match=r"nearest sizes that work: 80$"):
            StreamDoor(3, 44100, block_size=40, device=device)
        with pytest.raises(ValueError, match="LDS budget"):
            StreamDoor(3, 48000, block_size=8400, device=device)      # 16800 client samples per block
        for kw, match in ((dict(n_streams=0), "n_streams"), (dict(in_rate=0), "in_rate"), (dict(in_rate=44100.0), "in_rate"), (dict(out_rate=-8000), "out_rate"),
                          (dict(block_size=True), "block_size"), (dict(input_gain=float("nan")), "input_gain"), (dict(output_gain="3"), "output_gain")):
            args = dict(n_streams=3, in_rate=48000, device=device)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                StreamDoor(**args)
        # a well-formed door on the CPU - or on a GPU that is not there - is refused too, still without allocating
        if device == "cpu" or not torch.cuda.is_available():
            with pytest.raises(ValueError, match="lives on the GPU"):
                StreamDoor(3, 48000, device=device)


def test_stream_door_accepts_every_table_rate_at_the_default_block(lib, monkeypatch):
    """up to the device: the geometry a door would have is computed (and checked against the table) before the device is looked at"""
    from tinyvc_amd.module.infer import StreamDoor
    seen = {}
    real = stream_resample_geometry

    def spy(i, o, n, lib=None):
        seen[(i, o)] = (n,) + real(i, o, n, lib)
        return seen[(i, o)][1:]
    from tinyvc_amd.module.infer import stream as stream_mod
    monkeypatch.setattr(stream_mod, "stream_resample_geometry", spy)
    for in_freq, out_freq, _o, _n, _w, _t, _G, hist, delay, client in TABLE:
        rate = in_freq if out_freq == 24000 else out_freq
        with pytest.raises(ValueError, match="lives on the GPU"):
            StreamDoor(2, rate, device="cpu")
        n_in, n_out = (client, 1920) if out_freq == 24000 else (1920, client)
        assert seen[(in_freq, out_freq)] == (n_in, n_out, hist, delay)


def test_stream_classes_take_a_door():
    import inspect
    from tinyvc_amd.module.infer import BatchedStreamInfer, Generator, StreamInfer
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    for cls in (BatchedStreamInfer, StreamInfer):
        assert "door" in inspect.signature(cls.__init__).parameters and hasattr(cls, "audio_callback_pcm")
    st = BatchedStreamInfer(Generator(Encoder(), Decoder()), 2, device=torch.device("cpu"))
    assert st.door is None
    with pytest.raises(ValueError, match="needs a door"):
        st.audio_callback_pcm(torch.zeros(2, 3840, dtype=torch.int16))


# ---- infer_streaming.py --resample ---------------------------------------------------------------------------------------------------------
def _args(*argv):
    import infer_streaming
    return infer_streaming, infer_streaming.build_parser().parse_args(list(argv))


def test_cli_resample_argument_check(lib):
    m, args = _args("--resample", "-sr", "44100", "-c", "1920")
    with pytest.raises(SystemExit) as e:
        m.check_resample(args)
    assert "-c 1920 at -sr 44100 is not a multiple of 147" in str(e.value) and "1911 or 2058" in str(e.value)
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--resample", "-sr", "44100", "-c", "1920", "-encp", "/nonexistent/encoder.pt"])
    assert "not a multiple of 147" in str(e.value)
    m, args = _args("--resample", "-sr", "44100", "-c", "3528")
    assert m.check_resample(args) == 1920
    m, args = _args("--resample", "-sr", "48000", "-c", "3840")
    assert m.check_resample(args) == 1920
    m, args = _args("--resample")      # the defaults: 24 kHz, 1920
    assert m.check_resample(args) == 1920
    m, args = _args("-sr", "44100", "-c", "1920")      # without the flag nothing is checked or changed
    assert m.check_resample(args) is None and m.check_auto_pitch(args) is None
    for argv, text in ((("--resample", "-sr", "0"), "positive"), (("--resample", "-c", "-5"), "positive"), (("--resample", "-sr", "48000", "-c", "16800"), "LDS budget")):
        m, args = _args(*argv)
        with pytest.raises(SystemExit) as e:
            m.check_resample(args)
        assert text in str(e.value), (argv, str(e.value))
    # --auto-pitch counts frames of the model's block, not of -c
    m, args = _args("--resample", "-sr", "48000", "-c", "3840", "--auto-pitch")
    assert m.check_auto_pitch(args, m.check_resample(args))["new_frames"] == 4
