"""The streams' noise gate without a GPU: the geometry entry (tvc_stream_gate_geometry: no context, no device) and its messages, StreamGate's
and the stream constructors' refusals, the look-ahead-against-padding check, and infer_streaming.py's --gate flags with their rounding of
milliseconds to sub-frames.  Everything is refused on the host, before any device work."""
import ctypes
import inspect
import math
import types

import pytest
import torch

from tinyvc_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, *a):
    nsub, look = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.tvc_stream_gate_geometry(*a, ctypes.byref(nsub), ctypes.byref(look))
    return rc, nsub.value, look.value, lib.tvc_stream_gate_geometry_message(*a).decode()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_rule_and_messages(lib):
    # block, sub, look, hold, attack, release
    assert _geometry(lib, 1920, 240, 2, 20, 1, 10) == (0, 8, 480, "")
    assert _geometry(lib, 480, 120, 0, 0, 1, 1) == (0, 4, 0, "")
    assert _geometry(lib, 4, 4, 4095, 1 << 20, 1 << 20, 1 << 20) == (0, 1, 4095 * 4, "")
    assert _geometry(lib, 4096 * 65536, 65536, 0, 0, 1, 1) == (0, 4096, 0, "")
    assert lib.tvc_stream_gate_geometry(1920, 240, 2, 20, 1, 10, None, None) == 0      # the out pointers are optional
    for args, why in (((1920, 250, 0, 0, 1, 1), "sub = 250 is not a multiple of 4"),
                      ((1920, 0, 0, 0, 1, 1), "sub = 0 is outside 4 .. 65536"),
                      ((1 << 20, 1 << 17, 0, 0, 1, 1), "sub = 131072 is outside 4 .. 65536"),
                      ((1920, 256, 0, 0, 1, 1), "block = 1920 is not a whole number of 256-sample sub-frames"),
                      ((0, 240, 0, 0, 1, 1), "block = 0 is not positive"),
                      ((-240, 240, 0, 0, 1, 1), "block = -240 is not positive"),
                      ((1920, 240, -1, 0, 1, 1), "look = -1 is negative"),
                      ((1920, 240, 4089, 0, 1, 1), "block / sub + look = 4097 sub-frames is above 4096"),
                      ((4097 * 4, 4, 0, 0, 1, 1), "block / sub + look = 4097 sub-frames is above 4096"),
                      ((1920, 240, 0, -1, 1, 1), "hold = -1 is outside 0 .. 1048576"),
                      ((1920, 240, 0, (1 << 20) + 1, 1, 1), "hold = 1048577 is outside 0 .. 1048576"),
                      ((1920, 240, 0, 0, 0, 1), "attack = 0 is outside 1 .. 1048576"),
                      ((1920, 240, 0, 0, 1, 0), "release = 0 is outside 1 .. 1048576"),
                      ((1920, 240, 0, 0, 1, (1 << 20) + 1), "release = 1048577 is outside 1 .. 1048576")):
        rc, nsub, look, msg = _geometry(lib, *args)
        assert (rc, nsub, look) == (-1, -7, -7) and msg == why, (args, msg)
    assert _geometry(lib, 1920, 240, 4088, 0, 1, 1)[:2] == (0, 8)      # 8 + 4088 = 4096: the last that fits
    # the call itself wants a context before anything else
    assert lib.tvc_stream_gate_f32(None, None, None, 1, 0, None, None, None, 1, 1920, 240, 0, 0, 1, 1, 6.0, 0.0, None, None, None, None, None) == -1


def test_engine_wrapper_of_the_rule(lib):
    from tinyvc_amd import engine
    assert engine.stream_gate_geometry(1920, 240, 2, 20, 1, 10, lib) == (8, 480)
    assert engine.stream_gate_geometry(1920, 240, lib=lib) == (8, 0)
    with pytest.raises(ValueError, match="stream gate geometry: sub = 250 is not a multiple of 4"):
        engine.stream_gate_geometry(1920, 250, lib=lib)
    with pytest.raises(ValueError, match="look must be an integer"):
        engine.stream_gate_geometry(1920, 240, 1.5, lib=lib)
    with pytest.raises(ValueError, match="block must be an integer"):
        engine.stream_gate_geometry(True, 240, lib=lib)
    assert callable(engine.Engine.stream_gate)
    assert list(inspect.signature(engine.Engine.stream_gate).parameters)[1:6] == ["x", "y", "shift", "gate", "base"]


# ---- StreamGate --------------------------------------------------------------------------------------------------------------------------
def test_stream_gate_refuses_before_allocating(lib, monkeypatch):
    from tinyvc_amd.module.infer import StreamGate
    from tinyvc_amd.module.infer import stream as stream_mod

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    for name in ("zeros", "ones", "full", "tensor", "empty"):
        monkeypatch.setattr(stream_mod.torch, name, no_alloc)
    for device in ("cuda", "cpu"):
        for kw, match in ((dict(n_streams=0), "n_streams"), (dict(block_size=1920.0), "block_size"), (dict(sub_frame=True), "sub_frame"),
                          (dict(hold_size=100), "hold_size must be a whole number of 240-sample sub-frames"), (dict(hold_size=-240), "hold_size"),
                          (dict(attack_size=0), "attack_size .* at least 1"), (dict(release_size=0), "release_size .* at least 1"),
                          (dict(release_size=2400.0), "release_size"), (dict(lookahead_size=250), "lookahead_size"),
                          (dict(threshold_db=float("nan")), "threshold_db"), (dict(threshold_db="-40"), "threshold_db"),
                          (dict(threshold_db=[-40.0, -50.0]), r"one per stream \(3\)"), (dict(hysteresis_db=-1.0), "hysteresis_db"),
                          (dict(hysteresis_db=float("inf")), "hysteresis_db"), (dict(range_db=3.0), "range_db"), (dict(range_db=float("nan")), "range_db"),
                          (dict(block_size=1000), "StreamGate: stream gate geometry: block = 1000 is not a whole number of 240-sample sub-frames"),
                          (dict(sub_frame=250, hold_size=0, attack_size=250, release_size=250, lookahead_size=0, block_size=1000), "sub = 250 is not a multiple of 4"),
                          (dict(lookahead_size=240 * 4090), "block / sub \\+ look = 4098"), (dict(hold_size=240 * ((1 << 20) + 1)), "hold = 1048577")):
            args = dict(n_streams=3, block_size=1920, device=device)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                StreamGate(**args)
        # a well-formed gate on the CPU - or on a GPU that is not there - is refused too, still without allocating
        if device == "cpu" or not torch.cuda.is_available():
            for kw in (dict(), dict(threshold_db=-math.inf), dict(threshold_db=[-40.0, -45.0, -math.inf], range_db=-20.0, lookahead_size=0, hold_size=0)):
                with pytest.raises(ValueError, match="live on the GPU"):
                    StreamGate(3, 1920, device=device, **kw)
    sig = inspect.signature(StreamGate.__init__).parameters
    assert list(sig)[1:] == ["n_streams", "block_size", "threshold_db", "hysteresis_db", "hold_size", "attack_size", "release_size", "lookahead_size",
                             "sub_frame", "range_db", "device"]
    assert (sig["hysteresis_db"].default, sig["sub_frame"].default, sig["range_db"].default, sig["device"].default) == (6.0, 240, -math.inf, None)
    assert "guesses" in StreamGate.__doc__ and hasattr(StreamGate, "reset") and hasattr(StreamGate, "params")


# ---- the stream classes ------------------------------------------------------------------------------------------------------------------
def _gen():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def _fake_gate(n_streams, block_size, lookahead_size=0):
    """what the stream classes look at before any device work"""
    resets = []
    return types.SimpleNamespace(n_streams=n_streams, block_size=block_size, lookahead_size=lookahead_size, reset=lambda: resets.append(1), resets=resets)


def test_stream_classes_take_a_gate_and_refuse_a_foreign_one(lib):
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    cpu = torch.device("cpu")
    for cls in (BatchedStreamInfer, StreamInfer):
        p = inspect.signature(cls.__init__).parameters
        assert "gate" in p and p["gate"].default is None
    assert BatchedStreamInfer(_gen(), 2, device=cpu).gate is None
    with pytest.raises(ValueError, match="gate: built for 3 streams of 1920-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(_gen(), 2, device=cpu, gate=_fake_gate(3, 1920))
    with pytest.raises(ValueError, match="gate: built for 2 streams of 960-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(_gen(), 2, device=cpu, gate=_fake_gate(2, 960))
    with pytest.raises(ValueError, match="gate: built for 2 streams"):
        StreamInfer(_gen(), gate=_fake_gate(2, 1920))
    g = _fake_gate(2, 1920)
    st = BatchedStreamInfer(_gen(), 2, device=cpu, gate=g)
    assert st.gate is g and "gate" in st._graph_key.__doc__


def test_init_buffer_checks_the_look_ahead_against_the_padding(lib, monkeypatch):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    from tinyvc_amd.module.infer import stream as stream_mod
    from tinyvc_amd.module.infer.stream import check_gate_lookahead, check_window
    # the function: room = crossfade + delay - pad
    assert check_gate_lookahead(0, 240, 480, 0) == 720 and check_gate_lookahead(720, 240, 480, 0) == 720
    assert check_gate_lookahead(5760, 1920, 3840, 0) == 5760 and check_gate_lookahead(480, 240, 480, 240) == 480
    with pytest.raises(ValueError, match=r"lookahead_size = 721 is more than the 720 input samples .*crossfade_size 240 \+ last_delay_size 480 - pad_size 0"):
        check_gate_lookahead(721, 240, 480, 0)
    with pytest.raises(ValueError, match="lookahead_size = 720 is more than the 480 input samples"):
        check_gate_lookahead(720, 240, 480, 240)
    assert list(inspect.signature(check_window).parameters) == ["block_size", "extra_size", "crossfade_size", "sola_search_size", "last_delay_size", "auto_pitch"]
    # init_buffer: refused before a buffer exists; a window that is not whole frames takes its pad off the room
    cpu = torch.device("cpu")
    kw = dict(block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480)
    st = BatchedStreamInfer(_gen(), 2, device=cpu, extra_size=3840, gate=_fake_gate(2, 480, 960), **kw)      # a window of 4320: whole frames
    with pytest.raises(ValueError, match="lookahead_size = 960 is more than the 720"):
        st.init_buffer()
    assert not hasattr(st, "input_wav") and st.gate.resets == []
    st = BatchedStreamInfer(_gen(), 2, device=cpu, extra_size=3600, gate=_fake_gate(2, 480, 720), **kw)       # 4080: 240 samples of padding
    assert st.pad_size == 240
    with pytest.raises(ValueError, match="lookahead_size = 720 is more than the 480"):
        st.init_buffer()
    st.gate.lookahead_size = 480
    st.init_buffer()
    assert st.gate.resets == [1] and st.input_wav.shape == (2, 4080)
    st.gate = _fake_gate(3, 480)      # attributes are plain: a foreign gate put in later is met at the next init_buffer
    with pytest.raises(ValueError, match="gate: built for 3 streams"):
        st.init_buffer()


# ---- infer_streaming.py --gate -----------------------------------------------------------------------------------------------------------
def _args(*argv):
    import infer_streaming
    return infer_streaming, infer_streaming.build_parser().parse_args(list(argv))


def test_cli_gate_flags_and_rounding(lib):
    m, args = _args()
    assert args.gate is None and m.check_gate(args) is None      # absent: today's path
    m, args = _args("--gate", "-40")
    assert m.check_gate(args) == dict(threshold_db=-40.0, hysteresis_db=6.0, range_db=-math.inf, sub_frame=240, hold_size=4800, attack_size=240,
                                      release_size=2400, lookahead_size=480)
    # milliseconds -> whole 10 ms sub-frames, to the nearest; a fade takes at least one
    assert [m.gate_sub_frames(ms) for ms in (0, 4.9, 5.1, 10, 14.9, 15.1, 204, 1000)] == [0, 0, 1, 1, 1, 2, 20, 100]
    m, args = _args("--gate=-inf", "--gate-hysteresis", "3", "--gate-range", "-20", "--gate-hold", "204", "--gate-attack", "0", "--gate-release", "26",
                    "--gate-lookahead", "4")
    assert m.check_gate(args) == dict(threshold_db=-math.inf, hysteresis_db=3.0, range_db=-20.0, sub_frame=240, hold_size=4800, attack_size=240,
                                      release_size=720, lookahead_size=0)
    # the model's block, not -c, is what must be whole sub-frames
    m, args = _args("--gate", "-40", "--resample", "-sr", "48000", "-c", "3840")
    assert m.check_gate(args, m.check_resample(args))["sub_frame"] == 240
    for argv, text in ((("--gate-hold", "100"), "--gate-hold without --gate DB"),
                       (("--gate-range", "-20", "--gate-lookahead", "10"), "--gate-range --gate-lookahead without --gate DB"),
                       (("--gate", "nan"), "--gate: a threshold in dB"),
                       (("--gate", "-40", "--gate-hysteresis", "-1"), "--gate-hysteresis -1.0"),
                       (("--gate", "-40", "--gate-range", "6"), "--gate-range 6.0"),
                       (("--gate", "-40", "--gate-hold", "-5"), "--gate-hold -5.0"),
                       (("--gate", "-40", "--gate-release", "inf"), "--gate-release inf"),
                       (("--gate", "-40", "-c", "2000"), "blocks of 2000 samples at 24 kHz are not whole 240-sample (10 ms) sub-frames"),
                       (("--gate", "-40", "--gate-lookahead", "250"), "lookahead_size = 6000 is more than the 5760 input samples"),
                       (("--gate", "-40", "--crossfade", "240", "--lookahead", "0", "-e", "3840"), "lookahead_size = 480 is more than the 240"),
                       (("--gate", "-40", "--gate-hold", "20000000"), "hold = 2000000 is outside 0 .. 1048576")):
        m, args = _args(*argv)
        with pytest.raises(SystemExit) as e:
            m.check_gate(args)
        assert text in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--gate", "-40", "-c", "2000", "-encp", "/nonexistent/encoder.pt"])
    assert "not whole 240-sample" in str(e.value)
    text = m.build_parser().format_help()
    assert all(f in text for f in ("--gate DB", "--gate-hysteresis", "--gate-range", "--gate-hold", "--gate-attack", "--gate-release", "--gate-lookahead"))
    assert "guesses" in text
