"""tinyvc_amd.stream_state on CPU tensors: the four tables (what each stream stage keeps on the device) and the four functions that
allocate, reset, check and key a stage by its table; and engine.integer, the one integer check of the geometry calls."""
import types

import numpy as np
import pytest
import torch

from tinyvc_amd import stream_state as ss
from tinyvc_amd.engine import integer

S = 3
CPU = torch.device("cpu")
TABLES = {"door": ss.DOOR_STATE, "denoise": ss.DENOISE_STATE, "gate": ss.GATE_STATE, "track": ss.TRACK_STATE}
F32, I32, I64 = torch.float32, torch.int32, torch.int64
# the layout, written out once more by hand: (name, dtype, shape behind [S], start; None = a live parameter)
WANT = {
    "door": [("in_state", F32, (5,), 0.0), ("out_state", F32, (3,), 0.0)],
    "denoise": [("reduction_db", F32, (), None), ("hist", F32, (4,), 0.0), ("ola", F32, (4,), 0.0), ("smooth", F32, (321,), 0.0), ("noise", F32, (321,), 0.0),
                ("frames", I32, (), 0), ("noise_db", F32, (), -200.0)],
    "gate": [("threshold_db", F32, (), None), ("open", I32, (), 1), ("hold", I32, (), 0), ("gain", F32, (), 1.0), ("level_db", F32, (), -200.0)],
    "track": [("ring", F32, (8,), 0.0), ("count", I64, (), 0), ("auto", F32, (), 0.0)],
}


def _stage(table):
    """a bare object with the tail attributes, allocated by `table`, its live parameters filled as a stage class would"""
    ns = types.SimpleNamespace(n_streams=S, delay_size=4, hist_in=5, hist_out=3, window_frames=8)
    before = set(vars(ns))
    ss.allocate(ns, table, CPU)
    assert set(vars(ns)) - before == {f.name for f in table if f.start is not None}, "allocate sets the state and leaves a live parameter unset"
    for f in table:
        if f.start is None:
            setattr(ns, f.name, torch.tensor([-40.0, -50.0, -60.0]))
    return ns


def _scribble(ns, table):
    for i, f in enumerate(table):
        getattr(ns, f.name).copy_(torch.arange(getattr(ns, f.name).numel()).reshape(getattr(ns, f.name).shape) + 7 + i)
    return {f.name: getattr(ns, f.name).clone() for f in table}


@pytest.mark.parametrize("stage", sorted(TABLES))
def test_allocate_and_reset_follow_the_table(stage):
    table = TABLES[stage]
    assert [f.name for f in table] == [w[0] for w in WANT[stage]], "the fields, in the order the C entry takes them"
    ns = _stage(table)
    for f, (name, dtype, tail, start) in zip(table, WANT[stage]):
        t = getattr(ns, name)
        assert (f.dtype, f.start) == (dtype, start) and t.dtype == dtype and tuple(t.shape) == (S,) + tail and t.is_contiguous(), name
        if start is not None:
            assert bool((t == start).all()), name
    ptrs = ss.addresses(ns, table)
    assert ptrs == tuple(getattr(ns, f.name).data_ptr() for f in table)
    wrote = _scribble(ns, table)
    ss.reset(ns, table, streams=[1])
    for name, dtype, tail, start in WANT[stage]:
        t = getattr(ns, name)
        if start is None:
            assert torch.equal(t, wrote[name]), f"{name}: reset touched a live parameter"
            continue
        assert bool((t[1] == start).all()), f"{name}: row 1 is not back at the start"
        assert torch.equal(t[[0, 2]], wrote[name][[0, 2]]), f"{name}: reset([1]) touched a neighbour"
    ss.reset(ns, table)
    for name, dtype, tail, start in WANT[stage]:
        t = getattr(ns, name)
        assert torch.equal(t, wrote[name]) if start is None else bool((t == start).all()), name
    assert ss.addresses(ns, table) == ptrs, "reset works in place: a captured graph holds these addresses"


@pytest.mark.parametrize("stage", sorted(TABLES))
def test_checked_returns_the_tensors_in_order_and_names_what_it_refuses(stage):
    table = TABLES[stage]
    ns = _stage(table)
    got = ss.checked(ns, table, S, CPU, f"call: {stage}.")
    assert len(got) == len(table) and all(g is getattr(ns, f.name) for g, f in zip(got, table))
    for f in table:
        good = getattr(ns, f.name)
        wide = torch.zeros(S, 2 * good.shape[1], dtype=f.dtype)[:, ::2] if good.dim() == 2 else torch.zeros(S, 2, dtype=f.dtype)[:, 0]
        assert wide.shape == good.shape and not wide.is_contiguous()
        for bad in (good.to(torch.float64), torch.zeros((S + 1,) + tuple(good.shape[1:]), dtype=f.dtype), torch.zeros(S, 2, dtype=f.dtype),
                    wide, torch.empty(good.shape, dtype=f.dtype, device="meta"), None):
            setattr(ns, f.name, bad)
            with pytest.raises(ValueError, match=rf"call: {stage}\.{f.name} must be "):
                ss.checked(ns, table, S, CPU, f"call: {stage}.")
        setattr(ns, f.name, good)
    with pytest.raises(ValueError, match=rf"{table[0].name} must be contiguous torch.float32 \[4"):
        ss.checked(ns, table, S + 1, CPU, "")
    assert all(a is b for a, b in zip(ss.checked(ns, table, S, CPU, ""), got))


def test_the_integer_check():
    assert integer(np.int64(3), "sola", "delay") == 3 and type(integer(np.int64(3), "sola", "delay")) is int
    assert integer(-(2 ** 31) + 1, "sola", "delay") == -(2 ** 31) + 1
    for bad in (True, 1.5, 2 ** 31, -(2 ** 31), "3", None):
        with pytest.raises(ValueError, match="sola geometry: block must be an integer, got"):
            integer(bad, "sola geometry", "block")
