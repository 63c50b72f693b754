"""One speaker index per utterance, without a GPU: the new C symbols are exported and declared, refuse a null context before any
device work, and the Python surface rejects malformed multi-index targets and shift lists before it touches an engine."""
import ctypes

import pytest
import torch

from tinyvc_amd import _lib

NEW = ("tvc_knn_match_multi_f32", "tvc_workspace_bytes_multi", "tvc_convert_multi_f32", "tvc_workspace_bytes_ragged_multi",
       "tvc_convert_ragged_multi_f32")


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_null_context_is_refused_before_device_work(lib):
    n = (ctypes.c_int64 * 2)(300, 6000)
    blobs = (ctypes.c_void_p * 2)(256, 512)
    lens = (ctypes.c_int64 * 2)(4800, 9600)
    size = ctypes.c_size_t(0)
    assert lib.tvc_knn_match_multi_f32(None, None, None, blobs, n, None, None, 2, 10, None, 0) == -1
    assert lib.tvc_workspace_bytes_multi(None, 2, 4800, n, ctypes.byref(size)) == -1
    assert lib.tvc_convert_multi_f32(None, None, None, blobs, n, 0.0, None, None, 0, None, 2, 4800, None, 0) == -1
    assert lib.tvc_workspace_bytes_ragged_multi(None, 2, 9600, lens, n, ctypes.byref(size)) == -1
    assert lib.tvc_convert_ragged_multi_f32(None, None, None, 9600, lens, blobs, n, 0.0, None, None, 0, None, 2, None, 0) == -1
    assert size.value == 0


def _generator():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())          # on the CPU: any engine use would raise TinyVCError, not ValueError


@pytest.mark.parametrize("tgt", [
    [torch.zeros(1, 768, 10), torch.zeros(2, 768, 10)],            # an element that is not [1, 768, N]
    [torch.zeros(1, 768, 10), torch.zeros(1, 767, 10)],            # wrong feature size
    [torch.zeros(1, 768, 10), torch.zeros(1, 768, 3)],             # fewer than k = 4 vectors
    [torch.zeros(1, 768, 10), torch.zeros(1, 768, 10, dtype=torch.float64)],
    [torch.zeros(1, 768, 10)] * 3,                                 # three indices for two rows
    torch.zeros(3, 768, 10),                                       # the tensor form, three rows for two
    [],
    [torch.zeros(1, 768, 10), "index"],
])
def test_generator_rejects_malformed_targets_before_any_engine(tgt):
    gen = _generator()
    with pytest.raises(ValueError):
        gen.convert(torch.zeros(2, 4800), tgt, 0.0)


@pytest.mark.parametrize("shift", [[1.0, 2.0, 3.0], [1.0], torch.zeros(3), torch.zeros(2, 2)])
def test_generator_rejects_shift_lists_of_the_wrong_length(shift):
    gen = _generator()
    with pytest.raises(ValueError):
        gen.convert(torch.zeros(2, 4800), [torch.zeros(1, 768, 10)] * 2, shift)
    with pytest.raises(ValueError):
        gen.convert(torch.zeros(2, 4800), torch.zeros(1, 768, 10), shift)


def test_prepare_references_rejects_malformed_targets():
    from tinyvc_amd.module.tinyvc.feature_retrieval import check_references, prepare_references
    for bad in ([torch.zeros(768, 10)], torch.zeros(768, 10), torch.zeros(2, 768, 2), None, [torch.zeros(1, 768, 10), None]):
        with pytest.raises(ValueError):
            prepare_references(bad)
    assert check_references([torch.zeros(1, 768, 10), torch.zeros(1, 768, 20, dtype=torch.float16)]) == 2
    assert check_references(torch.zeros(5, 768, 10), 5) == 5
