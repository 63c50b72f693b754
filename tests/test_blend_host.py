"""A weighted blend of speaker indices, without a GPU: the new C symbols are declared, exported and bound and refuse a null context; the
Python surface (check_blend, Blend, Generator.convert) rejects malformed blends before it touches an engine; the entry scripts parse
`--blend PATH=W ...` and refuse a fifth entry or a missing weight."""
import ctypes
import os
import re

import pytest
import torch

from tinyvc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tvc_knn_match_blend_f32", "tvc_workspace_bytes_blend", "tvc_convert_blend_f32", "tvc_workspace_bytes_ragged_blend",
       "tvc_convert_ragged_blend_f32")


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_new_symbols_are_in_the_header_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in tinyvc_hip.h"
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+TVC_BLEND_MAX\s+4\b", header)


def test_null_context_is_refused_before_device_work(lib):
    n = (ctypes.c_int64 * 4)(300, 6000, 300, 6000)
    blobs = (ctypes.c_void_p * 4)(256, 512, 256, 512)
    lens = (ctypes.c_int64 * 2)(4800, 9600)
    size = ctypes.c_size_t(0)
    w = ctypes.c_void_p(1024)
    assert lib.tvc_knn_match_blend_f32(None, None, None, blobs, n, 2, w, None, None, 2, 10, None, 0) == -1
    assert lib.tvc_workspace_bytes_blend(None, 2, 4800, n, 2, ctypes.byref(size)) == -1
    assert lib.tvc_convert_blend_f32(None, None, None, blobs, n, 2, w, 0.0, None, None, 0, None, 2, 4800, None, 0) == -1
    assert lib.tvc_workspace_bytes_ragged_blend(None, 2, 9600, lens, n, 2, ctypes.byref(size)) == -1
    assert lib.tvc_convert_ragged_blend_f32(None, None, None, 9600, lens, blobs, n, 2, w, 0.0, None, None, 0, None, 2, None, 0) == -1
    assert size.value == 0


def _idx(n=10, rows=1, dtype=torch.float32):
    return torch.zeros(rows, 768, n, dtype=dtype)


BAD = {
    "M = 0": ([], []),
    "M = 5": ([_idx()] * 5, [0.2] * 5),
    "weights: three floats for two terms": ([_idx(), _idx()], [0.5, 0.3, 0.2]),
    "weights: a [3] tensor for two terms": ([_idx(), _idx()], torch.ones(3)),
    "weights: [2, 3] for two terms": ([_idx(), _idx()], torch.ones(2, 3)),
    "weights: [3, 2] for two rows": ([_idx(), _idx()], torch.ones(3, 2)),
    "weights: three dimensions": ([_idx(), _idx()], torch.ones(1, 2, 2)),
    "terms: three indices in a list for two rows": ([[_idx()] * 3, _idx()], [0.5, 0.5]),
    "terms: a [3, 768, N] tensor for two rows": ([_idx(), _idx(rows=3)], [0.5, 0.5]),
    "terms: row counts that disagree with each other": ([_idx(rows=2), [_idx()] * 3], [0.5, 0.5]),
    "terms: a non-tensor": ([_idx(), "index.pt"], [0.5, 0.5]),
    "terms: None": ([_idx(), None], [0.5, 0.5]),
    "terms: fewer than k = 4 vectors": ([_idx(), _idx(3)], [0.5, 0.5]),
    "terms: fp64": ([_idx(), _idx(dtype=torch.float64)], [0.5, 0.5]),
    "terms: not a list": (_idx(), [1.0]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_check_blend_refuses_malformed_blends_on_the_host(case):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, check_blend
    terms, weights = BAD[case]
    with pytest.raises(ValueError):
        check_blend(terms, weights, 2)
    with pytest.raises(ValueError):
        Blend(terms, weights).resolve(2, "cpu")      # (resolve checks first: no engine is reached)


def test_check_blend_accepts_every_form():
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, check_blend
    assert check_blend([_idx()], [1.0]) == (1, None)
    assert check_blend([_idx(), _idx(20, dtype=torch.float16)], (0.7, 0.3)) == (2, None)
    assert check_blend([_idx(), _idx(rows=3)], torch.ones(2)) == (2, 3)
    assert check_blend([[_idx(), _idx(12), _idx()], _idx()], torch.ones(3, 2), 3) == (2, 3)
    assert check_blend([_idx()] * 4, torch.ones(6, 4)) == (4, 6)
    b = Blend([_idx(), _idx()], [0.25, 0.75])
    assert b.M == 2 and b.rows is None and b.weights is None and len(b.term_tensors()) == 2      # nothing on a device yet


def test_generator_rejects_malformed_blends_before_any_engine():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Blend, Decoder, Encoder
    gen = Generator(Encoder(), Decoder())          # on the CPU: any engine use would raise TinyVCError, not ValueError
    wf = torch.zeros(2, 4800)
    with pytest.raises(ValueError):
        gen.convert(wf, Blend([_idx(), _idx(rows=3)], [0.5, 0.5]), 0.0)                  # three rows of indices for two utterances
    with pytest.raises(ValueError):
        gen.convert(wf, Blend([_idx(), _idx()], torch.ones(3, 2)), 0.0)                  # three rows of weights
    with pytest.raises(ValueError):
        gen.convert(wf, Blend([_idx(), _idx()], [0.5, 0.5]), [1.0, 2.0, 3.0])            # three shifts


@pytest.mark.parametrize("script", ["infer", "infer_streaming"])
def test_entry_scripts_parse_blend(script, capsys):
    mod = __import__(script)
    args = mod.build_parser().parse_args(["--blend", "a.pt=0.7", "b.pt=0.3"])
    assert args.blend == (["a.pt", "b.pt"], [0.7, 0.3])
    assert mod.build_parser().parse_args([]).blend is None
    assert mod.build_parser().parse_args(["--blend", "dir/x=y.pt=-0.5"]).blend == (["dir/x=y.pt"], [-0.5])
    for bad in (["a=1", "b=1", "c=1", "d=1", "e=1"], ["a.pt=0.7", "b.pt"], ["a.pt=heavy"], ["=1"]):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--blend"] + bad)
    assert "--blend" in capsys.readouterr().err
