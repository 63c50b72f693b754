"""The index-compaction surface without a GPU: the five new symbols are declared, exported and bound alike, every call refuses a NULL
context before any device work, and extract_index.py parses and checks its --compact flags before it loads anything."""
import ctypes
import os
import re

import pytest

from tinyvc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"tvc_ctx_set_index_assign_chunk": 2, "tvc_workspace_bytes_index_compact": 4, "tvc_index_assign_f32": 11, "tvc_index_update_f32": 10,
       "tvc_index_compact_f32": 14}


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_header_exports_and_ctypes_table_agree(lib):
    src = open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\b(tvc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))
    for name, nargs in NEW.items():
        assert name in protos, f"{name} is not declared in tinyvc_hip.h"
        assert len(protos[name].split(",")) == nargs
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert lib.tvc_version() == 1
    assert "extract_index.py:43-58" in open(os.path.join(ROOT, "include", "tinyvc_hip.h")).read()


def test_every_call_refuses_a_null_context(lib):
    need = ctypes.c_size_t()
    assert lib.tvc_ctx_set_index_assign_chunk(None, 512) == -1
    assert lib.tvc_workspace_bytes_index_compact(None, 1000, 10, ctypes.byref(need)) == -1
    assert lib.tvc_index_assign_f32(None, None, None, 1000, None, 10, None, None, None, None, 0) == -1
    assert lib.tvc_index_update_f32(None, None, None, 1000, None, 10, None, None, None, 0) == -1
    assert lib.tvc_index_compact_f32(None, None, None, 1000, None, 10, 1, None, None, None, None, None, None, 0) == -1


def test_cli_parses_and_checks_the_compact_flags():
    import extract_index
    a = extract_index.parse_args(["-size", "2048"])
    assert a.compact is None and a.compact_iters == 8 and a.compact_snap is False
    a = extract_index.parse_args(["-size", "2048", "--compact", "256", "--compact-iters", "3", "--compact-snap"])
    assert a.compact == 256 and a.compact_iters == 3 and a.compact_snap is True
    assert extract_index.parse_args(["-size", "256", "--compact", "256"]).compact == 256
    for bad in (["-size", "100", "--compact", "101"], ["-size", "100", "--compact", "3"], ["-size", "100", "--compact", "16", "--compact-iters", "0"],
                ["-size", "100", "--compact-snap"]):
        with pytest.raises(SystemExit):
            extract_index.parse_args(bad)
