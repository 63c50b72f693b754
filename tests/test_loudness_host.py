"""The loudness envelope match without a GPU: the geometry entries (no context, no device) and their messages, the new symbols in the header,
the binding and the library, LOUDNESS_STATE against a layout written out by hand, the refusals of LoudnessMatch / resolve_loudness /
StreamLoudness (all on the host, before anything is allocated), the new keyword in the three signatures, and the entry scripts' flags.
The fp64 restatement the GPU tests compare against (helpers_loudness) is held here against numbers worked out by hand."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import helpers_loudness as H
from tinyvc_amd import _lib
from tinyvc_amd import stream_state as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tvc_loudness_geometry", "tvc_loudness_geometry_message", "tvc_stream_loudness_geometry", "tvc_stream_loudness_geometry_message",
       "tvc_loudness_match_f32", "tvc_stream_loudness_f32")


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, length, sub, smooth):
    nsub, window, tile = ctypes.c_int64(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.tvc_loudness_geometry(length, sub, smooth, ctypes.byref(nsub), ctypes.byref(window), ctypes.byref(tile))
    return rc, nsub.value, window.value, tile.value, lib.tvc_loudness_geometry_message(length, sub, smooth).decode()


def _block_geometry(lib, block, sub, smooth):
    nsub, window = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.tvc_stream_loudness_geometry(block, sub, smooth, ctypes.byref(nsub), ctypes.byref(window))
    return rc, nsub.value, window.value, lib.tvc_stream_loudness_geometry_message(block, sub, smooth).decode()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_rule_and_messages(lib):
    rc, nsub, window, tile, msg = _geometry(lib, 96000, 240, 2)
    assert (rc, nsub, window, msg) == (0, 400, 5, "") and tile >= 1
    assert _geometry(lib, 30000 * 240, 240, 2)[:3] == (0, 30000, 5), "a five-minute row"
    assert _geometry(lib, 4, 4, 0)[:3] == (0, 1, 1) and _geometry(lib, 65536, 65536, 32)[:3] == (0, 1, 65)
    assert _geometry(lib, 1 << 40, 4, 0)[:2] == (0, 1 << 38)
    assert lib.tvc_loudness_geometry(1920, 240, 2, None, None, None) == 0      # the out pointers are optional
    for args, why in (((1920, 250, 2), "sub = 250 is not a multiple of 4"), ((1920, 0, 2), "sub = 0 is outside 4 .. 65536"),
                      ((1 << 20, 1 << 17, 2), "sub = 131072 is outside 4 .. 65536"), ((1920, 256, 2), "length = 1920 is not a whole number of 256-sample sub-frames"),
                      ((0, 240, 2), "length = 0 is outside 1 .. 1099511627776"), ((-240, 240, 2), "length = -240 is outside 1 .. 1099511627776"),
                      (((1 << 40) + 4, 4, 2), "length = 1099511627780 is outside 1 .. 1099511627776"),
                      ((1920, 240, -1), "smooth = -1 is outside 0 .. 32"), ((1920, 240, 33), "smooth = 33 is outside 0 .. 32")):
        rc, nsub, window, tile, msg = _geometry(lib, *args)
        assert (rc, nsub, window, tile) == (-1, -7, -7, -7) and msg == why, (args, msg)
    # a stream's block: the same rule, and at most 4096 sub-frames
    assert _block_geometry(lib, 1920, 240, 2) == (0, 8, 5, "") and _block_geometry(lib, 480, 240, 0) == (0, 2, 1, "")
    assert _block_geometry(lib, 4096 * 4, 4, 32) == (0, 4096, 65, "")
    for args, why in (((4097 * 4, 4, 2), "block / sub = 4097 sub-frames is above 4096"), ((1920, 250, 2), "sub = 250 is not a multiple of 4"),
                      ((1000, 240, 2), "length = 1000 is not a whole number of 240-sample sub-frames"), ((1920, 240, 33), "smooth = 33 is outside 0 .. 32")):
        rc, nsub, window, msg = _block_geometry(lib, *args)
        assert (rc, nsub, window) == (-1, -7, -7) and msg == why, (args, msg)
    # the device entries want a context before anything else
    assert lib.tvc_loudness_match_f32(None, None, None, None, None, 1, 240, None, None, 240, 2, -60.0, 12.0, 40.0, None) == -1
    assert lib.tvc_stream_loudness_f32(None, None, None, 1, 0, None, None, None, 1, 480, 240, 2, -60.0, 12.0, 40.0, None, None, None, None, None, None, None) == -1


def test_engine_wrappers_of_the_rule(lib):
    from tinyvc_amd import engine
    nsub, window, tile = engine.loudness_geometry(96000, lib=lib)
    assert (nsub, window) == (400, 5) and tile == _geometry(lib, 96000, 240, 2)[3]
    assert engine.loudness_geometry(1920, 240, 0, stream_block=True, lib=lib) == (8, 1, None)
    with pytest.raises(ValueError, match="loudness geometry: sub = 250 is not a multiple of 4"):
        engine.loudness_geometry(1920, 250, lib=lib)
    with pytest.raises(ValueError, match="loudness geometry: block / sub = 5000 sub-frames is above 4096"):
        engine.loudness_geometry(5000 * 240, 240, 2, stream_block=True, lib=lib)
    assert engine.loudness_geometry(5000 * 240, 240, 2, lib=lib)[0] == 5000
    for bad, name in (((1920.0, 240, 2), "length"), ((True, 240, 2), "length"), ((1920, 240.5, 2), "sub"), ((1920, 240, 1.5), "smooth")):
        with pytest.raises(ValueError, match=f"{name} must be an integer"):
            engine.loudness_geometry(*bad, lib=lib)
    assert engine.loudness_levels() == (-60.0, 12.0, 40.0) and engine.loudness_levels(-45.5, 0, 0) == (-45.5, 0.0, 0.0)
    for kw, text in ((dict(floor_db=math.nan), "floor_db must be a finite number of dB, got nan"), (dict(floor_db=-math.inf), "floor_db must be a finite"),
                     (dict(boost_db=-1.0), "boost_db must be a finite number of dB >= 0, got -1.0"), (dict(boost_db=math.inf), "boost_db must be a finite"),
                     (dict(cut_db=-0.5), "cut_db must be a finite number of dB >= 0"), (dict(cut_db=math.nan), "cut_db must be a finite"),
                     (dict(cut_db="40"), "cut_db must be a finite"), (dict(floor_db=True), "floor_db must be a finite"), (dict(floor_db=-601.0), "outside -600 .. 600"),
                     (dict(boost_db=1e39), "outside -600 .. 600")):
        with pytest.raises(ValueError, match=text):
            engine.loudness_levels(**kw)
    assert list(inspect.signature(engine.Engine.loudness_match).parameters)[1:] == ["x", "y", "share", "lengths", "settings", "out", "want_gains"]
    assert list(inspect.signature(engine.Engine.stream_loudness).parameters)[1:] == ["x", "y", "shift", "stage", "base", "out", "want_gains"]


def test_the_new_symbols_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^(int|const char\*) {name}\(", header, re.M), f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not listed in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], f"{name} is not exported by the library"
    # the binding's argument counts are the header's
    for name in NEW:
        decl = re.search(rf"{name}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "exactly 1" in header and "rounded to fp32 once" in header and "nobody has listened" in header


# ---- the state table -----------------------------------------------------------------------------------------------------------------------
F32, F64, I64 = torch.float32, torch.float64, torch.int64
WANT = [("share", F32, (), None), ("src_ring", F64, (5,), 0.0), ("out_ring", F64, (5,), 0.0), ("frames", I64, (), 0), ("gain", F32, (), 1.0),
        ("gain_db", F32, (), 0.0)]      # the layout, written out once more by hand: (name, dtype, shape behind [S], start; None = a live parameter)
S = 3
CPU = torch.device("cpu")


def _stage():
    ns = types.SimpleNamespace(n_streams=S, window=5)
    before = set(vars(ns))
    ss.allocate(ns, ss.LOUDNESS_STATE, CPU)
    assert set(vars(ns)) - before == {w[0] for w in WANT if w[3] is not None}, "allocate sets the state and leaves the live parameter unset"
    ns.share = torch.tensor([1.0, 0.5, 0.0])
    return ns


def test_the_state_table_against_a_layout_written_by_hand():
    table = ss.LOUDNESS_STATE
    assert [f.name for f in table] == [w[0] for w in WANT], "the fields, in the order the C entry takes them"
    ns = _stage()
    for f, (name, dtype, tail, start) in zip(table, WANT):
        t = getattr(ns, name)
        assert (f.dtype, f.start) == (dtype, start) and t.dtype == dtype and tuple(t.shape) == (S,) + tail and t.is_contiguous(), name
        if start is not None:
            assert bool((t == start).all()), name
    ptrs = ss.addresses(ns, table)
    assert ptrs == tuple(getattr(ns, f.name).data_ptr() for f in table)
    wrote = {}
    for i, f in enumerate(table):
        t = getattr(ns, f.name)
        t.copy_(torch.arange(t.numel()).reshape(t.shape) + 7 + i)
        wrote[f.name] = t.clone()
    ss.reset(ns, table, streams=[1])
    for name, dtype, tail, start in WANT:
        t = getattr(ns, name)
        if start is None:
            assert torch.equal(t, wrote[name]), f"{name}: reset touched a live parameter"
            continue
        assert bool((t[1] == start).all()), f"{name}: row 1 is not back at the start"
        assert torch.equal(t[[0, 2]], wrote[name][[0, 2]]), f"{name}: reset([1]) touched a neighbour"
    ss.reset(ns, table)
    for name, dtype, tail, start in WANT:
        t = getattr(ns, name)
        assert torch.equal(t, wrote[name]) if start is None else bool((t == start).all()), name
    assert ss.addresses(ns, table) == ptrs, "reset works in place: a captured graph holds these addresses"


def test_checked_returns_the_tensors_in_order_and_names_what_it_refuses():
    table = ss.LOUDNESS_STATE
    ns = _stage()
    got = ss.checked(ns, table, S, CPU, "stream_loudness: loudness.")
    assert len(got) == len(table) and all(g is getattr(ns, f.name) for g, f in zip(got, table))
    for f in table:
        good = getattr(ns, f.name)
        other = torch.float32 if f.dtype != torch.float32 else torch.float64
        for bad in (good.to(other), torch.zeros((S + 1,) + tuple(good.shape[1:]), dtype=f.dtype), torch.zeros(S, 2, dtype=f.dtype),
                    torch.empty(good.shape, dtype=f.dtype, device="meta"), None):
            setattr(ns, f.name, bad)
            with pytest.raises(ValueError, match=rf"stream_loudness: loudness\.{f.name} must be "):
                ss.checked(ns, table, S, CPU, "stream_loudness: loudness.")
        setattr(ns, f.name, good)
    ns.window = 3      # the rings follow the stage's window
    with pytest.raises(ValueError, match=r"src_ring must be contiguous torch.float64 \[3, 3\]"):
        ss.checked(ns, table, S, CPU, "")


# ---- LoudnessMatch, resolve_loudness, StreamLoudness ---------------------------------------------------------------------------------------
def test_loudness_match_and_resolve_refuse_on_the_host(lib):
    from tinyvc_amd.module.tinyvc.feature_retrieval import LoudnessMatch, resolve_loudness
    sig = inspect.signature(LoudnessMatch.__init__).parameters
    assert list(sig)[1:] == ["share", "sub_frame", "smooth", "floor_db", "boost_db", "cut_db"]
    assert [sig[k].default for k in list(sig)[2:]] == [240, 2, -60.0, 12.0, 40.0]
    assert "guesses" in LoudnessMatch.__doc__ and "nobody has listened" in LoudnessMatch.__doc__
    m = LoudnessMatch(0.5, sub_frame=120, smooth=0, floor_db=-50, boost_db=6, cut_db=20)
    assert (m.share, m.sub_frame, m.smooth, m.floor_db, m.boost_db, m.cut_db) == (0.5, 120, 0, -50.0, 6.0, 20.0)
    for kw, text in ((dict(sub_frame=250), "loudness: loudness geometry: sub = 250 is not a multiple of 4"), (dict(sub_frame=0), "sub = 0 is outside"),
                     (dict(sub_frame=240.0), "sub must be an integer"), (dict(smooth=33), "smooth = 33 is outside 0 .. 32"), (dict(smooth=-1), "smooth = -1"),
                     (dict(smooth=True), "smooth must be an integer"), (dict(floor_db=math.nan), "floor_db must be a finite"),
                     (dict(boost_db=-3), "boost_db must be a finite number of dB >= 0"), (dict(cut_db=math.inf), "cut_db must be a finite")):
        with pytest.raises(ValueError, match=text):
            LoudnessMatch(1.0, **kw)
    # the share: alpha's forms, by alpha's code; a bare value is LoudnessMatch(value)
    settings, share = resolve_loudness(0.25, 3)
    assert isinstance(settings, LoudnessMatch) and (settings.sub_frame, settings.smooth) == (240, 2) and share == [0.25] * 3
    assert resolve_loudness([0.0, 1.0], 2)[1] == [0.0, 1.0] and resolve_loudness(m, 2) == (m, [0.5, 0.5]) and resolve_loudness(1, 1)[1] == [1.0]
    for bad, text in ((1.5, r"loudness: a share of the source's envelope in \[0, 1\], got 1.5"), (-0.1, "in \\[0, 1\\]"), (math.nan, "in \\[0, 1\\]"),
                      ([0.5, 2.0], "in \\[0, 1\\]"), ([0.5] * 3, "loudness: 3 shares for a batch of 2"), ("1", "loudness: a float"), (True, "loudness: a float"),
                      (torch.zeros(2), "loudness: a tensor lives on the GPU"), (torch.zeros(2, dtype=torch.float64), "loudness: an fp32 tensor"),
                      (torch.zeros(3), "loudness: a tensor of 1 or B = 2 shares"), (LoudnessMatch(7.0), "in \\[0, 1\\]")):
        with pytest.raises(ValueError, match=text):
            resolve_loudness(bad, 2)


def test_convert_refuses_a_bad_loudness_before_any_engine_work():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    from tinyvc_amd.module.tinyvc.feature_retrieval import LoudnessMatch
    gen = Generator(Encoder(), Decoder())
    gen.engine = lambda *a, **k: pytest.fail("a refused call reached the engine")
    wf, tgt = torch.zeros(2, 4800), torch.zeros(1, 768, 8)
    for bad, text in ((1.5, "in \\[0, 1\\]"), (math.nan, "in \\[0, 1\\]"), ([0.5] * 3, "3 shares for a batch of 2"),
                      (LoudnessMatch(0.5, sub_frame=200), "sub_frame = 200 does not divide the 480-sample frames")):
        with pytest.raises(ValueError, match=text):
            gen.convert(wf, tgt, 0.0, loudness=bad)


def test_stream_loudness_refuses_before_allocating(lib, monkeypatch):
    from tinyvc_amd.module.infer import StreamLoudness, stream
    sig = inspect.signature(StreamLoudness.__init__).parameters
    assert list(sig)[1:] == ["n_streams", "block_size", "share", "sub_frame", "smooth", "floor_db", "boost_db", "cut_db", "device"]
    assert [sig[k].default for k in list(sig)[3:]] == [1.0, 240, 2, -60.0, 12.0, 40.0, None]
    assert "guesses" in StreamLoudness.__doc__ and hasattr(StreamLoudness, "reset") and hasattr(StreamLoudness, "params")
    monkeypatch.setattr(stream, "allocate", lambda *a, **k: pytest.fail("a refused stage allocated"))
    monkeypatch.setattr(stream, "gpu_device", lambda *a, **k: pytest.fail("a refused stage asked for its device"))
    for a, kw, text in (((0, 480), {}, "n_streams must be an integer >= 1"), ((2, 480.0), {}, "block_size must be an integer >= 1"), ((True, 480), {}, "n_streams"),
                        ((2, 480), dict(share=1.5), "share must be a number in \\[0, 1\\]"), ((2, 480), dict(share=math.nan), "share must be a number"),
                        ((2, 480), dict(share=[0.5] * 3), "one per stream \\(2\\)"), ((2, 480), dict(share="1"), "share must be a number"),
                        ((2, 500), {}, "StreamLoudness: loudness geometry: length = 500 is not a whole number of 240-sample sub-frames"),
                        ((2, 480), dict(sub_frame=250), "sub = 250 is not a multiple of 4"), ((2, 480), dict(smooth=33), "smooth = 33 is outside 0 .. 32"),
                        ((2, 4097 * 4), dict(sub_frame=4), "block / sub = 4097 sub-frames is above 4096"), ((2, 480), dict(sub_frame=2.5), "sub must be an integer"),
                        ((2, 480), dict(floor_db=math.inf), "StreamLoudness: floor_db must be a finite"), ((2, 480), dict(boost_db=-1), "StreamLoudness: boost_db"),
                        ((2, 480), dict(cut_db=math.nan), "StreamLoudness: cut_db")):
        with pytest.raises(ValueError, match=text):
            StreamLoudness(*a, **kw)


def _fake_stage(S, block):
    return types.SimpleNamespace(n_streams=S, block_size=block, resets=[], reset=lambda: None)


def test_the_new_keyword_in_the_three_signatures():
    from tinyvc_amd.module.infer import BatchedStreamInfer, Generator, StreamInfer
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    p = inspect.signature(Generator.convert).parameters
    assert "loudness" in p and p["loudness"].default is None
    for cls in (BatchedStreamInfer, StreamInfer):
        p = inspect.signature(cls.__init__).parameters
        assert "loudness" in p and p["loudness"].default is None
    gen = Generator(Encoder(), Decoder())
    st = BatchedStreamInfer(gen, 2, device=CPU)
    assert st.loudness is None and [s[0] for s in st._stages()] == []
    with pytest.raises(ValueError, match="loudness: built for 3 streams of 1920-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(gen, 2, device=CPU, loudness=_fake_stage(3, 1920))
    with pytest.raises(ValueError, match="loudness: built for 2 streams of 480-sample blocks"):
        BatchedStreamInfer(gen, 2, device=CPU, loudness=_fake_stage(2, 480))
    st = BatchedStreamInfer(gen, 2, device=CPU, loudness=_fake_stage(2, 1920), gate=_fake_stage(2, 1920), denoise=_fake_stage(2, 1920))
    assert [s[0] for s in st._stages()] == ["denoise", "loudness", "gate"], "the stage is listed between the suppressor and the gate"
    assert st._stages()[1][2] is ss.LOUDNESS_STATE


# ---- the entry scripts ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_of_infer_streaming(lib):
    import infer_streaming as m
    args = m.build_parser().parse_args([])
    assert args.loudness is None and m.check_loudness(args) is None      # absent: today's path
    args = m.build_parser().parse_args(["--loudness", "0.75"])
    assert m.check_loudness(args) == dict(share=0.75, sub_frame=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0)
    args = m.build_parser().parse_args(["--loudness", "1", "--loudness-window", "10", "--loudness-floor", "-50", "--loudness-boost", "6", "--loudness-cut", "0"])
    assert m.check_loudness(args) == dict(share=1.0, sub_frame=240, smooth=0, floor_db=-50.0, boost_db=6.0, cut_db=0.0)
    args = m.build_parser().parse_args(["--loudness", "0.5", "--resample", "-sr", "48000", "-c", "3840"])      # the model's block, not -c
    assert m.check_loudness(args, m.check_resample(args))["smooth"] == 2
    for argv, text in ((("--loudness-window", "30"), "--loudness-window without --loudness E"), (("--loudness-floor", "-50", "--loudness-cut", "3"),
                                                                                                  "--loudness-floor --loudness-cut without --loudness E"),
                       (("--loudness", "1.5"), "--loudness: a share in 0 .. 1"), (("--loudness", "nan"), "--loudness: a share in 0 .. 1"),
                       (("--loudness", "1", "--loudness-window", "40"), "--loudness-window 40: an odd number of 10 ms sub-frames"),
                       (("--loudness", "1", "--loudness-window", "25"), "--loudness-window 25: an odd number"),
                       (("--loudness", "1", "--loudness-window", "670"), "smooth = 33 is outside 0 .. 32"),
                       (("--loudness", "1", "--loudness-boost", "-2"), "boost_db must be a finite number of dB >= 0"),
                       (("--loudness", "1", "--loudness-floor", "nan"), "floor_db must be a finite"),
                       (("--loudness", "1", "-c", "2000"), "length = 2000 is not a whole number of 240-sample sub-frames")):
        args = m.build_parser().parse_args(list(argv))
        with pytest.raises(SystemExit) as e:
            m.check_loudness(args)
        assert text in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--loudness", "1", "-c", "2000", "-encp", "/nonexistent/encoder.pt"])
    assert "not a whole number of 240-sample" in str(e.value)
    text = m.build_parser().format_help()
    assert all(f in text for f in ("--loudness E", "--loudness-window", "--loudness-floor", "--loudness-boost", "--loudness-cut"))


def test_cli_flag_of_infer_and_the_keywords_it_adds(capsys):
    import infer
    from tinyvc_amd.module.tinyvc.feature_retrieval import alpha_keywords, loudness_keywords
    args = infer.build_parser().parse_args([])
    assert args.loudness is None and loudness_keywords(args, "infer.py") == {} and alpha_keywords(args, "infer.py") == {}, "absent: the calls are today's"
    args = infer.build_parser().parse_args(["--loudness", "0.5", "--alpha", "0.25"])
    assert loudness_keywords(args, "infer.py") == {"loudness": 0.5} and alpha_keywords(args, "infer.py") == {"alpha": 0.25}
    assert "rms mix rate 0.5" in capsys.readouterr().out
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit) as e:
            loudness_keywords(infer.build_parser().parse_args(["--loudness", bad]), "infer.py")
        assert "--loudness must be a share in 0 .. 1" in str(e.value)
    assert "--loudness E" in infer.build_parser().format_help() and "stream_kw" in inspect.signature(infer.convert_chunked).parameters


# ---- the restatement, against numbers worked out by hand -----------------------------------------------------------------------------------
def test_the_restatement_on_hand_worked_cases():
    sub = 4
    x = np.array([1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 0], dtype=np.float32)
    assert H.powers(x, sub).tolist() == [1.0, 4.0, 0.0]
    floor, lo, hi = H.constants()
    assert (floor, lo) == (1e-6, 0.01) and abs(hi - 3.9810717055349722) < 1e-15
    assert [H.share_value(e) for e in (-1.0, 0.0, 0.25, 1.0, 7.0, math.nan)] == [0.0, 0.0, 0.25, 1.0, 1.0, 0.0]
    assert H.gain(16.0, 1.0, 1, 1.0, (floor, lo, hi)) == np.float32(hi) and H.gain(4.0, 1.0, 1, 1.0, (floor, lo, hi)) == np.float32(2.0)
    assert H.gain(4.0, 1.0, 1, 0.5, (floor, lo, hi)) == np.float32(2.0 ** 0.5) and H.gain(1.0, 1e9, 1, 1.0, (floor, lo, hi)) == np.float32(0.01)
    assert H.gain(0.0, 0.0, 3, 1.0, (floor, lo, hi)) == 1.0 and H.gain(math.nan, 1.0, 1, 1.0, (floor, lo, hi)) == 1.0
    assert H.gain(1.0, math.inf, 1, 1.0, (floor, lo, hi)) == 1.0 and H.gain(16.0, 1.0, 1, 0.0, (floor, lo, hi)) == 1.0
    # y = x / 2 on three sub-frames, smooth = 1: every window's ratio is 4, the gain 2; the first sub-frame is flat
    y = x / 2
    edges = H.offline_edges(x, y, 1.0, sub=sub, smooth=1)
    assert edges.tolist() == [2.0, 2.0, 2.0, 2.0]
    assert H.ramp(y, edges, sub).tolist() == x.tolist()
    assert H.offline_edges(x, y, 1.0, length=8, sub=sub, smooth=1).tolist() == [2.0, 2.0, 2.0, 1.0], "the gain behind a row's length is 1"
    # the ramp: from 1 to 2 over four samples, each step an fp32 operation
    assert H.ramp(np.ones(4, np.float32), np.array([1.0, 2.0], np.float32), 4).tolist() == [1.25, 1.5, 1.75, 2.0]
    # a stream trails: its gain at sub-frame i is the offline gain at i - smooth where both windows are whole
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(4 * 12).astype(np.float32), rng.standard_normal(4 * 12).astype(np.float32)
    off = H.offline_edges(x, y, 1.0, sub=4, smooth=1)
    st = H.StreamRestatement(sub=4, smooth=1)
    got = np.concatenate([st.block(x[i:i + 8], y[i:i + 8], 0, 1.0)[1:] for i in range(0, 48, 8)])
    assert st.frames == 12 and got[2:].tolist() == off[2:12].tolist()
    assert H.ulps(np.float32([1.0, 2.0]), np.float32([1.0, np.nextafter(np.float32(2.0), np.float32(3.0))])) == 1
