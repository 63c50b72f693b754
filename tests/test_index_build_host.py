"""The column plan of the one-pass index build, on the host (feature_retrieval.index_columns): the reference's recipe
(extract_index.py:43-58: every stride-th frame of each clip in order, concatenated, index_select(perm), the first `size`) as a list of
columns into the packed features of a ragged encode.  Checked on a dummy packed tensor whose column c holds the value c."""
import pytest
import torch

from tinyvc_amd.module.tinyvc.feature_retrieval import index_columns


def recipe(packed, frames, stride, size, perm):
    """extract_index.py:47-58 with torch ops on the clips' own [1, C, T_b] tensors."""
    feats, off = [], 0
    for t in frames:
        feats.append(packed[None, :, off:off + t][:, :, ::stride])
        off += t
    feats = torch.cat(feats, dim=2)
    if perm is not None:
        feats = feats.index_select(2, perm)
    return feats[:, :, :size] if size is not None else feats


def packed_of(frames):
    S = sum(frames)
    return torch.arange(S, dtype=torch.float32).repeat(3, 1)       # [3, S], column c holds c


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("size", [7, 30, 10000, None])              # smaller and larger than the supply, and "all"
def test_columns_reproduce_the_recipe(stride, size):
    frames = [50, 3, 65, 41, 4, 5]                                  # a 3-frame clip (the shortest the encoder takes), lengths on both sides of a stride multiple
    packed = packed_of(frames)
    supply = sum(-(-t // stride) for t in frames)
    perm = torch.randperm(supply, generator=torch.Generator().manual_seed(7))
    for pm in (perm, None):
        cols = index_columns(frames, stride, size, pm)
        want = recipe(packed, frames, stride, size, pm)
        assert cols.dtype == torch.int64 and cols.dim() == 1 and cols.is_contiguous()
        assert cols.numel() == want.shape[2] == (min(size, supply) if size is not None else supply)
        assert torch.equal(packed[:, cols][None], want)
        assert torch.equal(cols.float(), want[0, 0])                # the column numbers themselves, in the index's order


def test_one_three_frame_clip():
    assert index_columns([3], 4, None).tolist() == [0]
    assert index_columns([3], 1, 2).tolist() == [0, 1]
    assert index_columns([3, 3], 2, None, torch.tensor([3, 0])).tolist() == [5, 0]


def test_a_repeated_selection_is_allowed():
    """perm is an index list: index_select takes repeats, and so does the gather."""
    assert index_columns([8], 4, None, torch.tensor([1, 1, 0])).tolist() == [4, 4, 0]


@pytest.mark.parametrize("perm", [[0, 13], [-1, 0], [5, 2, 99]])
def test_out_of_range_selection_is_refused_on_the_host(perm):
    frames = [50]                                                   # 13 strided frames: 0 .. 12
    with pytest.raises(ValueError):
        index_columns(frames, 4, None, torch.tensor(perm))


@pytest.mark.parametrize("frames,stride,size", [([0, 5], 4, None), ([5], 0, None), ([5], 4, -1)])
def test_malformed_plans_are_refused(frames, stride, size):
    with pytest.raises(ValueError):
        index_columns(frames, stride, size)
