"""The SOLA geometry without a GPU: the host entry (tvc_sola_geometry: no context, no device), engine.sola_geometry, the fade window's
length at every legal cross-fade, the stream classes' constructor checks and infer_streaming.py's three flags.  Everything is refused on
the host, before any device work."""
import ctypes
import inspect
import math

import pytest
import torch

from tinyvc_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, block, cross, search, delay):
    min_ly, lo, hi = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.tvc_sola_geometry(block, cross, search, delay, ctypes.byref(min_ly), ctypes.byref(lo), ctypes.byref(hi))
    return rc, min_ly.value, lo.value, hi.value


# (block, cross, search, delay) -> what the message must name; None = legal
ROWS = [
    ((1, 4, 0, 0), None),
    ((1920, 1920, 1920, 3840), None),
    ((480, 240, 240, 480), None),
    ((1920, 0, 1920, 3840), "cross = 0"),
    ((1920, 2, 1920, 3840), "cross = 2"),
    ((1920, 6, 1920, 3840), "cross = 6"),
    ((1920, 1924, 1920, 3840), "cross = 1924"),
    ((1920, 1920, -1, 3840), "search = -1"),
    ((1920, 1920, 1921, 3840), "search = 1921"),
    ((1920, 1920, 1920, -1), "delay = -1"),
    ((0, 1920, 1920, 3840), "block = 0"),
]


@pytest.mark.parametrize("row,named", ROWS, ids=["-".join(str(v) for v in r[0]) for r in ROWS])
def test_geometry_row_by_row(lib, row, named):
    from tinyvc_amd.engine import sola_geometry
    block, cross, search, delay = row
    if named is None:
        want = (block + cross + search + delay, cross + delay, cross + search + delay)
        assert _geometry(lib, *row) == (0,) + want
        assert sola_geometry(*row, lib=lib) == want
        assert lib.tvc_sola_geometry_message(*row) == b""
        assert lib.tvc_sola_geometry(*row, None, None, None) == 0      # the out pointers are optional
    else:
        assert _geometry(lib, *row) == (-1, -1, -1, -1), "a refusal writes nothing"
        assert named in lib.tvc_sola_geometry_message(*row).decode()
        with pytest.raises(ValueError, match=named):
            sola_geometry(*row, lib=lib)


def test_geometry_corners_by_value(lib):
    assert _geometry(lib, 1, 4, 0, 0) == (0, 5, 4, 4)
    assert _geometry(lib, 1920, 1920, 1920, 3840) == (0, 9600, 5760, 7680)      # 240 .. 320 ms at 24 kHz
    assert _geometry(lib, 480, 240, 240, 480) == (0, 1440, 720, 960)            # 30 .. 40 ms
    from tinyvc_amd.engine import sola_geometry
    assert sola_geometry(1920) == (9600, 5760, 7680)                            # the defaults are the reference's
    for bad in (1.5, "4", True, None, 2 ** 31):
        with pytest.raises(ValueError, match="must be an integer"):
            sola_geometry(1920, bad)
    # a refused call without a context where one is needed
    assert lib.tvc_sola_geom_f32(None, None, None, None, None, None, None, 1, 9600, 1920, 1920, 1920, 3840, 0) == -1


def test_fade_window_has_exactly_cross_entries():
    """The reference's torch.arange(0, 1, 1 / cross) has cross + 1 entries for some sizes (a floating-point step); the window is its first
    cross entries, and at 1920 it is the reference's expression to the bit."""
    from tinyvc_amd.module.infer.stream import _fade_windows
    long = []
    for cross in range(4, 1921, 4):
        fi, fo = _fade_windows(cross, "cpu")
        assert fi.shape == fo.shape == (cross,), cross
        ref = torch.sin(math.pi * torch.arange(0, 1, 1 / cross) / 2) ** 2
        if ref.numel() != cross:
            long.append(cross)
        assert torch.equal(fi, ref[:cross]) and torch.equal(fo, 1 - ref[:cross])
    assert 196 in long and 1916 in long, "the sizes this test is about exist on this host"
    ref = torch.sin(math.pi * torch.arange(0, 1, 1 / 1920) / 2) ** 2
    assert ref.numel() == 1920 and torch.equal(_fade_windows(1920, "cpu")[0], ref)


# ---- the stream classes ----------------------------------------------------------------------------------------------------------------------
def _gen():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_stream_classes_take_the_geometry_keywords(lib):
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    for cls in (BatchedStreamInfer, StreamInfer):
        names = list(inspect.signature(cls.__init__).parameters)
        # behind every keyword the reference has and behind `door`; only auto_pitch / pitch_track, which tests/test_pitch_track_host.py holds last, follow
        assert names[-5:-2] == ["crossfade_size", "sola_search_size", "last_delay_size"] and names[-6] == "door"
        sig = inspect.signature(cls.__init__).parameters
        assert (sig["crossfade_size"].default, sig["sola_search_size"].default, sig["last_delay_size"].default) == (1920, 1920, 3840)
    cpu = torch.device("cpu")
    st = BatchedStreamInfer(_gen(), 2, device=cpu)
    assert (st.crossfade_size, st.sola_search_size, st.last_dilay_size, st.input_size) == (1920, 1920, 3840, 13440)
    assert st.latency_samples == (5760, 7680) and st.latency_seconds == (0.24, 0.32)
    st = BatchedStreamInfer(_gen(), 2, device=cpu, block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3840)
    assert (st.crossfade_size, st.sola_search_size, st.last_dilay_size) == (240, 240, 480) and not hasattr(st, "last_delay_size")
    assert st.input_size == 4320 and st.latency_samples == (720, 960) and st.latency_seconds == (0.03, 0.04)
    st = BatchedStreamInfer(_gen(), 2, device=cpu, block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480)
    assert st.input_size == 480 + 240 + 240 + 2 * 480      # the reference's formula over the attributes
    assert st._graph_key.__doc__ and "geometry" in st._graph_key.__doc__


def test_stream_constructor_refuses_before_device_work(lib, monkeypatch):
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    from tinyvc_amd.module.infer import stream as stream_mod

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    gen = _gen()
    monkeypatch.setattr(stream_mod.torch, "zeros", no_alloc)
    monkeypatch.setattr(type(gen), "engine", no_alloc)
    cpu = torch.device("cpu")
    for kw, named in ((dict(crossfade_size=6), "cross = 6"), (dict(crossfade_size=1924), "cross = 1924"), (dict(crossfade_size=0), "cross = 0"),
                      (dict(sola_search_size=-1), "search = -1"), (dict(sola_search_size=1921), "search = 1921"), (dict(last_delay_size=-1), "delay = -1"),
                      (dict(block_size=0), "block = 0"), (dict(crossfade_size=240.0), "must be an integer")):
        with pytest.raises(ValueError, match=named):
            BatchedStreamInfer(gen, 2, device=cpu, **kw)
        with pytest.raises(ValueError, match=named):
            StreamInfer(gen, device=cpu, **kw)
    # a window the front end cannot reflect-pad: 480 + 100 + 100 + 2 * 100 = 880 <= 960
    with pytest.raises(ValueError, match=r"window of 880 samples .* raise extra_size to more than 480"):
        BatchedStreamInfer(gen, 2, device=cpu, block_size=480, crossfade_size=100, sola_search_size=100, last_delay_size=100)
    with pytest.raises(ValueError, match="window of 960 samples"):
        BatchedStreamInfer(gen, 2, device=cpu, block_size=480, crossfade_size=100, sola_search_size=100, last_delay_size=100, extra_size=480)
    # 961 samples are converted as 1440: 479 samples of converted padding behind a look-ahead of 100 would reach into the emitted block
    with pytest.raises(ValueError, match=r"window of 961 samples is converted as 1440 .* extra_size = 960 makes the window whole frames"):
        BatchedStreamInfer(gen, 2, device=cpu, block_size=480, crossfade_size=100, sola_search_size=100, last_delay_size=100, extra_size=481)
    assert BatchedStreamInfer(gen, 2, device=cpu, block_size=480, crossfade_size=100, sola_search_size=100, last_delay_size=100, extra_size=960).input_size == 1440
    # a pad no longer than the look-ahead is legal, and the latency is that much shorter: 4420 samples are converted as 4800
    st = BatchedStreamInfer(gen, 2, device=cpu, block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3940)
    assert (st.input_size, st.pad_size, st.latency_samples) == (4420, 380, (340, 580))
    st = BatchedStreamInfer(gen, 2, device=cpu, block_size=1000)      # the default geometry with an odd block: 12520 -> 12960
    assert (st.input_size, st.pad_size, st.latency_samples) == (12520, 440, (5760 - 440, 7680 - 440))
    # the tracker's new frames end last_delay_size before the end of the window, in whole frames
    with pytest.raises(ValueError, match="last_delay_size = 500 is not a whole number of 480-sample frames"):
        BatchedStreamInfer(gen, 2, device=cpu, auto_pitch=True, last_delay_size=500)
    assert BatchedStreamInfer(gen, 2, device=cpu, auto_pitch=None, last_delay_size=500).last_dilay_size == 500
    assert BatchedStreamInfer(gen, 2, device=cpu, auto_pitch=True, last_delay_size=960).last_dilay_size == 960


# ---- infer_streaming.py --crossfade / --sola-search / --lookahead -----------------------------------------------------------------------------
def _args(*argv):
    import infer_streaming
    return infer_streaming, infer_streaming.build_parser().parse_args(list(argv))


def test_cli_geometry_check(lib):
    m, args = _args()
    assert (args.crossfade, args.sola_search, args.lookahead) == (1920, 1920, 3840) and m.check_geometry(args) == (5760, 7680)
    m, args = _args("-c", "480", "--crossfade", "240", "--sola-search", "240", "--lookahead", "480")
    assert m.check_geometry(args) == (720, 960)
    for argv, text in ((("--crossfade", "6"), "cross = 6"), (("--crossfade", "1924"), "cross = 1924"), (("--crossfade", "0"), "cross = 0"),
                       (("--sola-search", "-1"), "search = -1"), (("--sola-search", "1921"), "search = 1921"), (("--lookahead", "-1"), "delay = -1"),
                       (("-c", "0"), "block = 0"),
                       (("-c", "480", "-e", "0", "--crossfade", "100", "--sola-search", "100", "--lookahead", "100"), "raise extra_size to more than 480"),
                       (("-c", "480", "-e", "481", "--crossfade", "100", "--sola-search", "100", "--lookahead", "100"), "extra_size = 960 makes the window whole frames")):
        m, args = _args(*argv)
        with pytest.raises(SystemExit) as e:
            m.check_geometry(args)
        assert str(e.value).startswith("infer_streaming.py: ") and text in str(e.value), (argv, str(e.value))
    m, args = _args("--auto-pitch", "--lookahead", "500")
    with pytest.raises(SystemExit) as e:
        m.check_geometry(args)
    assert "--lookahead 500" in str(e.value) and "last_delay_size = 500 is not a whole number of 480-sample frames" in str(e.value)
    m, args = _args("--lookahead", "500")      # without the tracker any look-ahead goes; the 6760-sample window is converted as 7200
    assert m.check_geometry(args) == (1920 + 500 - 440, 1920 + 1920 + 500 - 440)
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--crossfade", "6", "-encp", "/nonexistent/encoder.pt"])
    assert "cross = 6" in str(e.value)
    with pytest.raises(SystemExit) as e:
        m.main(["--auto-pitch", "--lookahead", "500", "-encp", "/nonexistent/encoder.pt"])
    assert "--lookahead 500" in str(e.value)
    # with --resample the block is the model's, not -c
    m, args = _args("--resample", "-sr", "48000", "-c", "960", "--crossfade", "240", "--sola-search", "240", "--lookahead", "480")
    assert m.check_geometry(args, m.check_resample(args)) == (720, 960)
