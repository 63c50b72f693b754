"""The C ABI boundary, without a GPU: libtinyvc_hip.so loads, exports every prototype declared in
include/tinyvc_hip.h, and the ctypes table in tinyvc_amd/_lib.py mirrors the header one to one."""
import ctypes
import os
import re

import pytest

from tinyvc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    return {name: [a.strip() for a in args.split(",")] if args.strip() != "void" else [] for name, args in protos}


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)          # hipcc cross-compiles for gfx950 without a GPU
    return _lib.load_library()


def test_every_declared_symbol_is_exported(lib):
    decl = header_functions()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in tinyvc_hip.h but not exported"


def test_ctypes_table_matches_header(lib):
    decl = header_functions()
    assert set(decl) == set(_lib.SIGNATURES), set(decl) ^ set(_lib.SIGNATURES)
    for name, args in decl.items():
        assert len(args) == len(_lib.SIGNATURES[name][1]), f"{name}: header has {len(args)} parameters"


def test_prototypes_carry_the_headers_parameter_names():
    """every function's parameters are declared under the header's names, in the header's order: a pointer swapped with its neighbour no
    longer passes; and SIGNATURES, which load_library declares, is nothing but PROTOTYPES without the names"""
    decl = header_functions()
    assert set(decl) == set(_lib.PROTOTYPES)
    for name, args in decl.items():
        names = [re.findall(r"[A-Za-z_]\w*", a)[-1] for a in args]
        assert [n for n, _t in _lib.PROTOTYPES[name][1]] == names, name
    assert _lib.SIGNATURES == {name: (res, [t for _n, t in params]) for name, (res, params) in _lib.PROTOTYPES.items()}


# the conversion ladder: the 16 conversions, their 14 workspace queries, the 5 matches
LADDER = sorted(n for n in _lib.PROTOTYPES if re.fullmatch(
    r"tvc_convert\w*_f32|tvc_knn_match(_multi|_blend|_alpha|_protect)?_f32|tvc_workspace_bytes(_ragged)?(_multi|_blend|_auto|_alpha|_protect|_path)?", n))


def test_the_ladder_is_whole():
    assert [sum(n.startswith(p) for n in LADDER) for p in ("tvc_convert", "tvc_workspace_bytes", "tvc_knn_match")] == [16, 14, 5]


@pytest.mark.parametrize("entry", LADDER)
def test_arguments_orders_values_by_name(entry):
    """_lib.arguments: the entry's declared names, each with a sentinel of its own, come back in the header's order whatever else the dict
    holds at its "off" value; a declared name without a value raises, and so does a value the entry has no parameter for"""
    names = [re.findall(r"[A-Za-z_]\w*", a)[-1] for a in header_functions()[entry]]
    everything = {n for e in LADDER for n, _t in _lib.PROTOTYPES[e][1]}
    named = {n: off for n, off in zip(sorted(everything - set(names)), [None, 0, 0.0] * len(everything))}
    named.update((n, object()) for n in names)
    assert _lib.arguments(entry, named) == tuple(named[n] for n in names)
    assert _lib.arguments(entry, {n: named[n] for n in names}) == tuple(named[n] for n in names)
    for n in names:
        with pytest.raises(TypeError, match=f"`{n}`"):
            _lib.arguments(entry, {k: v for k, v in named.items() if k != n})
    for n in sorted(everything - set(names)):
        for on in (1, 0.5, object()):
            with pytest.raises(TypeError, match=f"`{n}`"):
                _lib.arguments(entry, dict(named, **{n: on}))


def test_arguments_refuses_alpha_at_the_multi_entry():
    named = dict.fromkeys((n for n, _t in _lib.PROTOTYPES["tvc_convert_multi_f32"][1]), 1)
    assert len(_lib.arguments("tvc_convert_multi_f32", dict(named, alpha=None))) == len(named)
    with pytest.raises(TypeError, match="tvc_convert_multi_f32 has no parameter `alpha`"):
        _lib.arguments("tvc_convert_multi_f32", dict(named, alpha=ctypes.c_void_p(4096)))


def test_version_and_null_safety(lib):
    assert lib.tvc_version() == 1
    # header + raw rows [N][768] + the bf16x3 image of the normalised vectors (1.5 floats per value) + inverse norms + their fp16 image
    assert lib.tvc_knn_prepared_elems(1000) == 64 + 1000 * 768 + 768 * 1024 * 3 // 2 + 1024 + 768 * 1024 // 2
    # fp16 storage: header + inverse norms [Npad] + the fp16 image (half a float per value): 2 B per element
    assert lib.tvc_knn_prepared_elems_f16(1000) == 64 + 1024 + 768 * 1024 // 2 + 8
    assert lib.tvc_knn_prepared_elems_f16(1000000) * 4 < 1.55e9
    assert lib.tvc_knn_prepared_elems(0) == 0
    # argument validation happens before any device work
    assert lib.tvc_finalize_weights(None) == -1
    assert lib.tvc_profile_enable(None, 1) == -1
    assert lib.tvc_last_error(None) == b"null ctx"


def test_no_cpu_fallback_in_product_path():
    """The product package never imports the oracle and fails loudly off-GPU."""
    import torch
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    from tinyvc_amd.module import utils
    with pytest.raises(_lib.TinyVCError):
        Encoder().infer(torch.zeros(1, 961, 4))
    with pytest.raises(_lib.TinyVCError):
        Decoder().infer(torch.zeros(1, 768, 4), torch.zeros(1, 1, 4), torch.zeros(1, 1, 1920))
    with pytest.raises(_lib.TinyVCError):
        utils.spectrogram(torch.zeros(1, 4800))
    for dirpath, _d, files in os.walk(os.path.join(ROOT, "tinyvc_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f"{f} imports the oracle"


def test_host_helpers():
    import torch
    from tinyvc_amd.engine import pitch_class_table
    from tinyvc_amd.module import utils
    t = pitch_class_table()
    assert t.shape == (512,) and t[0] == 0 and abs(float(t[48]) - 40.0) < 1e-4 and float(t[1]) > 20.0
    x = torch.ones(2, 1000)
    y = utils.autopad_waveform(x)
    assert y.shape == (2, 1440) and float(y[:, 1000:].abs().sum()) == 0 and utils.autopad_waveform(y) is y


def test_ragged_plan_is_host_logic(lib):
    """tvc_ragged_plan needs no context and no device: the split of a ragged call into in-kernel batches (length classes at 11 / 43 / 128
    frames - the kernels a FilterNet level runs depend on the utterance's length there -, a frame cap per batch), and its validation."""
    import ctypes

    def plan(frames, lmax_frames=None, cap=0):
        B = len(frames)
        lens = (ctypes.c_int64 * B)(*[480 * f for f in frames])
        out = (ctypes.c_int32 * B)()
        n = ctypes.c_int()
        rc = lib.tvc_ragged_plan(B, 480 * (lmax_frames or max(frames)), lens, cap, out, ctypes.byref(n))
        return rc, list(out), n.value

    rc, rows, n = plan([200, 5, 131, 10, 11, 42, 43, 127, 128, 3])
    assert rc == 0 and n == 4
    cls = lambda f: (f >= 11) + (f >= 43) + (f >= 128)
    frames = [200, 5, 131, 10, 11, 42, 43, 127, 128, 3]
    by_batch = {}
    for f, r in zip(frames, rows):
        by_batch.setdefault(r, set()).add(cls(f))
    assert all(len(v) == 1 for v in by_batch.values()) and len(by_batch) == 4      # one class per batch
    assert rows[0] == rows[2] == rows[8] == 0                                       # the longest class runs first
    rc, rows, n = plan([150] * 7)
    assert rc == 0 and n == 1 and rows == [0] * 7
    assert plan([2, 50])[0] != 0                                                    # 960 samples: too short for the STFT's reflect padding
    assert plan([50, 60], lmax_frames=55)[0] != 0                                   # longer than its row
    assert plan([90000])[0] != 0                                                    # longer than a batch may be
    rc, rows, n = plan([150] * 7, cap=400)
    assert rc == 0 and n == 4 and rows == [0, 0, 1, 1, 2, 2, 3]                     # the cap cuts a class into several batches, in order
    assert plan([150] * 7, cap=-1)[0] != 0
    assert lib.tvc_ctx_set_ragged_batch_frames(None, 400) == -1                     # the cap is a property of a context: no process-wide state
