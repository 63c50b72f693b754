"""The look-ahead peak limiter without a GPU: the geometry entries (no context, no device) and their messages, the new symbols in the
header, the binding and the library, LIMITER_STATE through allocate / reset / checked, the refusals of Limiter / resolve_limit /
StreamLimiter (all on the host, before anything is allocated), the new keywords, the entry scripts' flags with -og's way into the drive -
and the properties the kernels rest on, shown on the numpy restatement the GPU tests compare against (helpers_limiter): the recurrence
forgets within R + 1 steps for every legal R, the ceiling holds exactly, and a stream is the offline result one sub-frame late."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import helpers_limiter as H
from tinyvc_amd import _lib
from tinyvc_amd import stream_state as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tvc_limiter_geometry", "tvc_limiter_geometry_message", "tvc_stream_limiter_geometry", "tvc_stream_limiter_geometry_message", "tvc_limit_f32",
       "tvc_stream_limit_f32")
F = np.float32
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _geometry(lib, length, sub, release, stream=False):
    nsub, delay, tile = (ctypes.c_int if stream else ctypes.c_int64)(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    name = "tvc_stream_limiter_geometry" if stream else "tvc_limiter_geometry"
    rc = getattr(lib, name)(length, sub, release, ctypes.byref(nsub), ctypes.byref(delay), ctypes.byref(tile))
    return rc, nsub.value, delay.value, tile.value, getattr(lib, name + "_message")(length, sub, release).decode()


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_rule_and_messages(lib):
    rc, nsub, delay, tile, msg = _geometry(lib, 96000, 24, 100)
    assert (rc, nsub, delay, msg) == (0, 4000, 24, "") and tile >= 1
    assert _geometry(lib, 4, 4, 1)[:3] == (0, 1, 4) and _geometry(lib, 65536, 65536, 4096)[:3] == (0, 1, 65536) and _geometry(lib, 1 << 40, 4, 1)[:2] == (0, 1 << 38)
    assert lib.tvc_limiter_geometry(1920, 24, 100, None, None, None) == 0      # the out pointers are optional
    for args, why in (((1920, 26, 100), "sub = 26 is not a multiple of 4"), ((1920, 0, 100), "sub = 0 is outside 4 .. 65536"),
                      ((1 << 20, 1 << 17, 2), "sub = 131072 is outside 4 .. 65536"), ((1000, 24, 100), "length = 1000 is not a whole number of 24-sample sub-frames"),
                      ((0, 24, 100), "length = 0 is outside 1 .. 1099511627776"), (((1 << 40) + 4, 4, 2), "length = 1099511627780 is outside 1 .. 1099511627776"),
                      ((1920, 24, 0), "release = 0 is outside 1 .. 4096 sub-frames"), ((1920, 24, 4097), "release = 4097 is outside 1 .. 4096 sub-frames")):
        rc, nsub, delay, tile, msg = _geometry(lib, *args)
        assert (rc, nsub, delay, tile) == (-1, -7, -7, -7) and msg == why, (args, msg)
    # a stream's block: at least one sub-frame, whole sub-frames; the third value is the chunk the kernel walks a block in
    rc, nsub, delay, chunk, msg = _geometry(lib, 1920, 24, 100, stream=True)
    assert (rc, nsub, delay, msg) == (0, 80, 24, "") and chunk >= 1
    assert _geometry(lib, 1 << 30, 4, 1, stream=True)[:2] == (0, 1 << 28), "no resource depends on the block"
    for args, why in (((20, 24, 100), "block = 20 is outside one sub-frame .. 1073741824"), ((0, 24, 100), "block = 0 is outside one sub-frame .. 1073741824"),
                      ((1000, 24, 100), "block = 1000 is not a whole number of 24-sample sub-frames"), ((1920, 24, 5000), "release = 5000 is outside 1 .. 4096 sub-frames"),
                      ((1920, 22, 100), "sub = 22 is not a multiple of 4")):
        rc, nsub, delay, chunk, msg = _geometry(lib, *args, stream=True)
        assert (rc, nsub, delay, chunk) == (-1, -7, -7, -7) and msg == why, (args, msg)
    # the device entries want a context before anything else
    assert lib.tvc_limit_f32(None, None, None, None, 1, 24, None, None, 24, 100, 0.0, None) == -1
    assert lib.tvc_stream_limit_f32(None, None, None, None, 1, 24, 24, 100, 0.0, None, None, None, None, None, None) == -1


def test_engine_wrappers_of_the_rule(lib):
    from tinyvc_amd import engine
    assert engine.limiter_geometry(96000, lib=lib)[:2] == (4000, 24) and engine.limiter_geometry(1920, 24, 100, stream_block=True, lib=lib)[:2] == (80, 24)
    with pytest.raises(ValueError, match="limiter geometry: sub = 26 is not a multiple of 4"):
        engine.limiter_geometry(1920, 26, lib=lib)
    with pytest.raises(ValueError, match="limiter geometry: block = 1000 is not a whole number"):
        engine.limiter_geometry(1000, stream_block=True, lib=lib)
    for bad, name in (((1920.0, 24, 2), "length"), ((True, 24, 2), "length"), ((1920, 24.5, 2), "sub"), ((1920, 24, 1.5), "release")):
        with pytest.raises(ValueError, match=f"{name} must be an integer"):
            engine.limiter_geometry(*bad, lib=lib)
    assert engine.limiter_drive() == 0.0 and engine.limiter_drive(6) == 6.0
    for bad, text in ((math.nan, "drive_db must be a finite"), (math.inf, "drive_db must be a finite"), ("6", "drive_db must be a finite"), (True, "drive_db must be"),
                      (700.0, "outside -600 .. 600")):
        with pytest.raises(ValueError, match=text):
            engine.limiter_drive(bad)
    assert list(inspect.signature(engine.Engine.limit).parameters)[1:] == ["y", "ceiling", "lengths", "settings", "want_gains"]
    assert list(inspect.signature(engine.Engine.stream_limit).parameters)[1:] == ["y", "stage", "want_gains"]


def test_the_new_symbols_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^(int|const char\*) {name}\(", header, re.M), f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not listed in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], f"{name} is not exported by the library"
        decl = re.search(rf"{name}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "instant fall, linear rise" in header and "nobody has listened" in header and "32767 / 32768" in header and "margin, not proof" in header


# ---- the state table -----------------------------------------------------------------------------------------------------------------------
F32 = torch.float32
WANT = [("ceiling", F32, (), None), ("tail", F32, (24,), 0.0), ("peak", F32, (), 0.0), ("gain", F32, (), 1.0), ("reduction_db", F32, (), 0.0)]
S = 3


def _stage():
    ns = types.SimpleNamespace(n_streams=S, sub_frame=24)
    before = set(vars(ns))
    ss.allocate(ns, ss.LIMITER_STATE, CPU)
    assert set(vars(ns)) - before == {w[0] for w in WANT if w[3] is not None}, "allocate sets the state and leaves the live parameter unset"
    ns.ceiling = torch.tensor([0.5, 0.9, math.inf])
    return ns


def test_the_state_table_through_allocate_reset_and_checked():
    table = ss.LIMITER_STATE
    assert [f.name for f in table] == [w[0] for w in WANT], "the fields, in the order the C entry takes them"
    assert table[0].start is None, "the ceiling is a live parameter"
    ns = _stage()
    for f, (name, dtype, tail, start) in zip(table, WANT):
        t = getattr(ns, name)
        assert (f.dtype, f.start) == (dtype, start) and t.dtype == dtype and tuple(t.shape) == (S,) + tail and t.is_contiguous(), name
    ptrs = ss.addresses(ns, table)
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
        assert bool((t[1] == start).all()) and torch.equal(t[[0, 2]], wrote[name][[0, 2]]), name
    ss.reset(ns, table)
    assert all(torch.equal(getattr(ns, n), wrote[n]) if s is None else bool((getattr(ns, n) == s).all()) for n, _, _, s in WANT)
    assert ss.addresses(ns, table) == ptrs, "reset works in place: a captured graph holds these addresses"
    got = ss.checked(ns, table, S, CPU, "stream_limit: limiter.")
    assert len(got) == len(table) and all(g is getattr(ns, f.name) for g, f in zip(got, table))
    for f in table:
        good = getattr(ns, f.name)
        for bad in (good.double(), torch.zeros((S + 1,) + tuple(good.shape[1:])), torch.zeros(S, 2), None):
            setattr(ns, f.name, bad)
            with pytest.raises(ValueError, match=rf"stream_limit: limiter\.{f.name} must be "):
                ss.checked(ns, table, S, CPU, "stream_limit: limiter.")
        setattr(ns, f.name, good)
    ns.sub_frame = 48      # the tail follows the stage's sub-frame
    with pytest.raises(ValueError, match=r"tail must be contiguous torch.float32 \[3, 48\]"):
        ss.checked(ns, table, S, CPU, "")


# ---- Limiter, resolve_limit, StreamLimiter -------------------------------------------------------------------------------------------------
def test_limiter_and_resolve_limit_refuse_on_the_host(lib):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Limiter, limit_ceiling, resolve_limit
    sig = inspect.signature(Limiter.__init__).parameters
    assert list(sig)[1:] == ["ceiling_db", "sub_frame", "release_size", "drive_db"] and [sig[k].default for k in list(sig)[1:]] == [-1.0, 24, 2400, 0.0]
    assert "guesses" in Limiter.__doc__ and "nobody has listened" in Limiter.__doc__
    m = Limiter(-3, sub_frame=48, release_size=480, drive_db=6)
    assert (m.ceiling_db, m.sub_frame, m.release, m.release_size, m.drive_db) == (-3, 48, 10, 480, 6.0) and Limiter().release == 100
    for kw, text in ((dict(sub_frame=26), "limit: limiter geometry: sub = 26 is not a multiple of 4"), (dict(sub_frame=0), "sub_frame|sub = 0"),
                     (dict(sub_frame=24.0), "sub must be an integer"), (dict(release_size=2401), "release_size = 2401 is not a whole number of 24-sample sub-frames"),
                     (dict(release_size=0), "release = 0 is outside 1 .. 4096"), (dict(release_size=4097 * 24), "release = 4097 is outside"),
                     (dict(release_size=True), "release_size must be an integer"), (dict(drive_db=math.nan), "limit: drive_db must be a finite"),
                     (dict(drive_db=601), "outside -600 .. 600")):
        with pytest.raises(ValueError, match=text):
            Limiter(-1.0, **kw)
    # the ceiling: dBFS in alpha's forms, converted to linear once, in double, here; a tensor holds linear values already
    assert limit_ceiling(0) == 1.0 and limit_ceiling(math.inf) == math.inf and limit_ceiling(-20.0) == 10.0 ** -1.0
    settings, ceiling = resolve_limit(-1.0, 3)
    assert isinstance(settings, Limiter) and (settings.sub_frame, settings.release) == (24, 100) and ceiling == [10.0 ** (-1.0 / 20.0)] * 3
    assert resolve_limit([0.0, math.inf], 2)[1] == [1.0, math.inf] and resolve_limit(m, 2) == (m, [10.0 ** (-3 / 20.0)] * 2)
    for bad, text in ((math.nan, "limit: a ceiling is a number of dBFS"), (-math.inf, "limit: a ceiling is a number of dBFS"), (700.0, "in -600 .. 600"),
                      ([-1.0] * 3, "limit: 3 shares for a batch of 2"), ("-1", "limit: a float"), (True, "limit: a float"),
                      (torch.zeros(2), "limit: a tensor lives on the GPU"), (torch.zeros(2, dtype=torch.float64), "limit: an fp32 tensor"),
                      (torch.zeros(3), "limit: a tensor of 1 or B = 2"), (Limiter(math.nan), "a ceiling is a number of dBFS")):
        with pytest.raises(ValueError, match=text):
            resolve_limit(bad, 2)


def test_convert_refuses_a_bad_limit_before_any_engine_work():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    from tinyvc_amd.module.tinyvc.feature_retrieval import Limiter
    assert inspect.signature(Generator.convert).parameters["limit"].default is None
    gen = Generator(Encoder(), Decoder())
    gen.engine = lambda *a, **k: pytest.fail("a refused call reached the engine")
    wf, tgt = torch.zeros(2, 4800), torch.zeros(1, 768, 8)
    for bad, text in ((math.nan, "a ceiling is a number of dBFS"), ([-1.0] * 3, "3 shares for a batch of 2"),
                      (Limiter(-1.0, sub_frame=36, release_size=360), "sub_frame = 36 does not divide the 480-sample frames")):
        with pytest.raises(ValueError, match=text):
            gen.convert(wf, tgt, 0.0, limit=bad)


def test_stream_limiter_refuses_before_allocating(lib, monkeypatch):
    from tinyvc_amd.module.infer import StreamLimiter, stream
    sig = inspect.signature(StreamLimiter.__init__).parameters
    assert list(sig)[1:] == ["n_streams", "block_size", "ceiling_db", "sub_frame", "release_size", "drive_db", "device"]
    assert [sig[k].default for k in list(sig)[3:]] == [-1.0, 24, 2400, 0.0, None]
    assert "guesses" in StreamLimiter.__doc__ and "32767 / 32768" in StreamLimiter.__doc__ and "margin, not proof" in StreamLimiter.__doc__
    assert all(hasattr(StreamLimiter, k) for k in ("reset", "params", "set_ceiling_db"))
    monkeypatch.setattr(stream, "allocate", lambda *a, **k: pytest.fail("a refused stage allocated"))
    monkeypatch.setattr(stream, "gpu_device", lambda *a, **k: pytest.fail("a refused stage asked for its device"))
    for a, kw, text in (((0, 480), {}, "n_streams must be an integer >= 1"), ((2, 480.0), {}, "block_size must be an integer >= 1"), ((True, 480), {}, "n_streams"),
                        ((2, 480), dict(ceiling_db=math.nan), "ceiling_db must be a number of dBFS"), ((2, 480), dict(ceiling_db=[-1.0] * 3), "one per stream \\(2\\)"),
                        ((2, 480), dict(ceiling_db="-1"), "ceiling_db must be a number"), ((2, 480), dict(ceiling_db=-math.inf), "StreamLimiter: a ceiling is a number of dBFS"),
                        ((2, 500), {}, "StreamLimiter: limiter geometry: block = 500 is not a whole number of 24-sample sub-frames"),
                        ((2, 480), dict(sub_frame=26), "sub = 26 is not a multiple of 4"), ((2, 480), dict(release_size=2401), "release_size = 2401 is not a whole"),
                        ((2, 480), dict(release_size=4097 * 24), "release = 4097 is outside"), ((2, 480), dict(sub_frame=2.5), "sub must be an integer"),
                        ((2, 480), dict(drive_db=math.inf), "StreamLimiter: drive_db must be a finite")):
        with pytest.raises(ValueError, match=text):
            StreamLimiter(*a, **kw)


def _fake_stage(S, block, **kw):
    return types.SimpleNamespace(n_streams=S, block_size=block, reset=lambda: None, **kw)


def test_the_new_keyword_in_the_stream_classes():
    from tinyvc_amd.module.infer import BatchedStreamInfer, Generator, StreamInfer, StreamLimiter
    from tinyvc_amd.module.infer.stream import DOOR_CEILING_DB
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    import tinyvc_amd.module.infer as pkg
    assert "StreamLimiter" in pkg.__all__ and pkg.StreamLimiter is StreamLimiter
    for cls in (BatchedStreamInfer, StreamInfer):
        p = inspect.signature(cls.__init__).parameters
        assert "limiter" in p and p["limiter"].default is None
    gen = Generator(Encoder(), Decoder())
    st = BatchedStreamInfer(gen, 2, device=CPU)
    assert st.limiter is None and [s[0] for s in st._stages()] == [] and st.latency_samples == (5760, 7680)
    with pytest.raises(ValueError, match="limiter: built for 3 streams of 1920-sample blocks, the streams are 2 of 1920"):
        BatchedStreamInfer(gen, 2, device=CPU, limiter=_fake_stage(3, 1920))
    lim = _fake_stage(2, 1920, delay_size=24, ceiling_db=[-1.0, -1.0])
    st = BatchedStreamInfer(gen, 2, device=CPU, limiter=lim, gate=_fake_stage(2, 1920), loudness=_fake_stage(2, 1920))
    assert [s[0] for s in st._stages()] == ["loudness", "gate", "limiter"], "the stage is the last one"
    assert st._stages()[2][2] is ss.LIMITER_STATE and st.latency_samples == (5760 + 24, 7680 + 24)
    # in front of a door a ceiling above 32767 / 32768 bounds nothing: refused, here and in set_ceiling_db later
    assert DOOR_CEILING_DB == -0.001 and 10.0 ** (DOOR_CEILING_DB / 20.0) < 32767 / 32768
    door = _fake_stage(2, 1920, latency_seconds=0.0)
    with pytest.raises(ValueError, match="limiter: ceiling_db = 0 is above -0.001: the door's int16 conversion wraps"):
        BatchedStreamInfer(gen, 2, device=CPU, door=door, limiter=_fake_stage(2, 1920, delay_size=24, ceiling_db=[-1.0, 0.0]))
    st = BatchedStreamInfer(gen, 2, device=CPU, door=door, limiter=lim)
    assert lim.max_ceiling_db == DOOR_CEILING_DB
    real = object.__new__(StreamLimiter)      # (no device here: the host half of set_ceiling_db alone)
    real.max_ceiling_db = DOOR_CEILING_DB
    with pytest.raises(ValueError, match="ceiling_db = 0 is above -0.001: these streams end in a door"):
        real._ceilings(0.0, 2)
    assert real._ceilings([-6.0, -0.001], 2) == ([-6.0, -0.001], [10.0 ** (-6.0 / 20.0), 10.0 ** (-0.001 / 20.0)])


# ---- the entry scripts ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_of_infer_streaming(lib):
    import infer_streaming as m
    args = m.build_parser().parse_args(["-og", "6"])
    assert args.limit is None and m.check_limit(args) is None      # absent: today's path, -og stays the door's
    args = m.build_parser().parse_args(["--limit"])
    assert args.limit == -1.0 and m.check_limit(args) == dict(ceiling_db=-1.0, sub_frame=24, release_size=2400, drive_db=0.0)
    args = m.build_parser().parse_args(["--limit", "-3", "--limit-release", "50", "-og", "6"])      # -og becomes the drive in front of the limiter
    assert m.check_limit(args) == dict(ceiling_db=-3.0, sub_frame=24, release_size=1200, drive_db=6.0)
    args = m.build_parser().parse_args(["--limit", "--resample", "-sr", "48000", "-c", "3840"])      # the model's block, not -c
    assert m.check_limit(args, m.check_resample(args))["release_size"] == 2400
    for argv, text in ((("--limit-release", "30"), "--limit-release without --limit"), (("--limit", "0"), "--limit: a ceiling in dBFS of at most -0.001"),
                       (("--limit", "nan"), "at most -0.001"), (("--limit", "-700"), "at most -0.001"),
                       (("--limit", "--limit-release", "2.5"), "--limit-release 2.5: a whole number of 1 ms sub-frames"),
                       (("--limit", "--limit-release", "5000"), "release = 5000 is outside 1 .. 4096"), (("--limit", "--limit-release", "0"), "release = 0 is outside"),
                       (("--limit", "-c", "2000"), "block = 2000 is not a whole number of 24-sample sub-frames"), (("--limit", "-og", "nan"), "-og: drive_db must be a finite")):
        args = m.build_parser().parse_args(list(argv))
        with pytest.raises(SystemExit) as e:
            m.check_limit(args)
        assert text in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit) as e:      # main() gets no further than the check: nothing is loaded
        m.main(["--limit", "-c", "2000", "-encp", "/nonexistent/encoder.pt"])
    assert "not a whole number of 24-sample" in str(e.value)
    text = m.build_parser().format_help()
    assert "--limit [DB]" in text and "--limit-release MS" in text and "nobody has listened" in m.__doc__ and "margin, not proof" in m.__doc__


def test_cli_flag_of_infer_and_the_keywords_it_adds(capsys):
    import infer
    from tinyvc_amd.module.tinyvc.feature_retrieval import limit_keywords
    args = infer.build_parser().parse_args([])
    assert args.limit is None and limit_keywords(args, "infer.py") == {}, "absent: the calls are today's"
    assert limit_keywords(infer.build_parser().parse_args(["--limit"]), "infer.py") == {"limit": -1.0}
    assert limit_keywords(infer.build_parser().parse_args(["--limit", "-6.5", "--loudness", "0.5"]), "infer.py") == {"limit": -6.5}
    assert "-6.5 dBFS" in capsys.readouterr().out
    for bad in ("nan", "-700", "700"):
        with pytest.raises(SystemExit) as e:
            limit_keywords(infer.build_parser().parse_args(["--limit", bad]), "infer.py")
        assert "infer.py: --limit: a ceiling is a number of dBFS" in str(e.value)
    assert "--limit [DB]" in infer.build_parser().format_help()


# ---- the properties the kernels rest on, on the restatement ---------------------------------------------------------------------------------
def test_the_recurrence_forgets_within_release_plus_one_steps_for_every_release():
    """f(e) = min(1, e + d), d = 1.0f / R: f^(R+1)(0) == 1.0f exactly for R = 1 .. 4096 - what lets a tile start from e = 1 at R + 1 edges
    in front of it"""
    R = np.arange(1, 4097)
    d = (F(1) / R.astype(F)).astype(F)
    e = np.zeros(4096, F)
    steps = np.zeros(4096, np.int64)
    for i in range(4098):
        steps += e < 1
        e = np.minimum(F(1), (e + d).astype(F))
    assert bool((e == 1).all()) and bool((steps <= R + 1).all()), f"R = {R[steps > R + 1][:5]} need more than R + 1 steps"
    assert int((steps == R + 1).sum()) > 0, "R + 1 is needed for some R: R steps would not do"
    print(f"{int((steps == R + 1).sum())} of 4096 releases need R + 1 steps, the others R")


def test_the_restatement_on_hand_worked_cases():
    sub = 4
    y = np.array([0.5, -0.5, 0.25, 0, 2, -1, 0, 0, 0.5, 0, 0, 0], F)
    assert H.peaks(y, sub).tolist() == [0.5, 2.0, 0.5] and H.peaks(np.array([np.nan, 1, -3, np.nan], F), 4).tolist() == [3.0]
    r = H.ratios(H.peaks(y, sub), F(1.0))
    assert r.tolist() == [1.0, 0.5, 0.5, 1.0]
    assert H.recurrence(r, 4).tolist() == [1.0, 0.5, 0.5, 0.75]      # instant fall, linear rise by 1 / 4
    out, g = H.limit(y, 1.0, sub, 4)
    assert g.tolist() == [1.0, 0.5, 0.5, 0.75] and out[:4].tolist() == [0.5 * 0.875, -0.5 * 0.75, 0.25 * 0.625, 0.0] and out[4:8].tolist() == [1.0, -0.5, 0.0, 0.0]
    assert H.ratios(np.array([np.inf], F), F(1.0)).tolist() == [0.0, 0.0] and H.ratios(np.array([5.0], F), H.ceiling_of(np.inf)).tolist() == [1.0, 1.0]
    assert [float(H.ceiling_of(c)) for c in (0.5, 0.0, -1.0, math.nan, math.inf)] == [0.5, math.inf, math.inf, math.inf, math.inf]
    assert H.drive_of(0.0) == 1.0 and H.drive_of(20.0) == 10.0
    out, g = H.limit(y, 1.0, sub, 4, length=9)      # a ragged row owns whole sub-frames; behind them y's bits and gains of 1
    assert g.tolist() == [1.0, 0.5, 0.5, 1.0] and out[8:].tolist() == y[8:].tolist()


@pytest.mark.parametrize("sub,release,drive_db", [(4, 1, 0.0), (4, 3, 0.0), (4, 37, 6.0), (24, 100, -3.0)])
def test_the_ceiling_holds_exactly_and_a_restart_changes_no_bit(sub, release, drive_db):
    rng = np.random.default_rng(sub + release)
    K = 3 * release + 400
    for trial in range(3):
        y = H.bursty(rng, K * sub, sub, bursts=rng.integers(0, K, 12))
        c = F(rng.uniform(0.05, 0.9))
        out, g = H.limit(y, c, sub, release, drive_db)
        assert bool((np.abs(out) <= c).all()) and float(np.abs(out).max()) >= 0.99 * float(c) and g.min() < 0.5
        v = (y * H.drive_of(drive_db)).astype(F)
        r = H.ratios(H.peaks(v, sub), c)
        for k in rng.integers(release + 2, K, 8):      # from e = 1 at R + 1 edges back: the same gains from edge k on
            again = H.recurrence(r, release, F(1), start=int(k) - (release + 1))
            assert np.array_equal(H.bits(again[k:]), H.bits(g[k:])), f"restart in front of edge {k}"
        if drive_db == 0.0:      # where both edge gains are 1 the samples keep their bits (a ceiling between the noise and the bursts)
            out, g = H.limit(y, 2.0, sub, release)
            flat = (g[:-1] == 1) & (g[1:] == 1)
            assert flat.any() and not flat.all() and np.array_equal(H.bits(out.reshape(K, sub)[flat]), H.bits(y.reshape(K, sub)[flat]))


@pytest.mark.parametrize("per", [1, 2, 7])
def test_a_stream_restatement_is_the_offline_one_a_sub_frame_late(per):
    sub, release = 4, 5
    rng = np.random.default_rng(per)
    K = 14 * 9
    y = H.bursty(rng, K * sub, sub, bursts=[0, 3, 40, 41, 90, K - 1])
    out, g = H.limit(y, 0.4, sub, release, 2.0)
    st, outs, edges = H.Stream(sub, release, 2.0), [], [np.ones(1, F)]
    for i in range(0, K * sub, per * sub):
        o, e = st.block(y[i:i + per * sub], 0.4)
        outs.append(o)
        edges.append(e[1:])
    assert np.array_equal(H.bits(np.concatenate(outs)), H.bits(np.concatenate([np.zeros(sub, F), out[:-sub]])))
    assert np.array_equal(H.bits(np.concatenate(edges)[1:]), H.bits(g[:-1]))
    assert st.gain == g[K - 1] and np.array_equal(H.bits(st.tail), H.bits((y[-sub:] * H.drive_of(2.0)).astype(F)))
