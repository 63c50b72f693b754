"""The device state of the per-stream stages, declared once: which tensors a stage owns, their dtype, their shape behind [n_streams] and
what a fresh stream starts from.  The stage classes allocate and reset by these tables, the engine checks a stage against its table and
passes the tensors on in table order - the order the C entry takes them -, and a captured stream graph is keyed by their addresses: a
tensor that reaches the library is in the table, so it is checked, reset and keyed.  The stages are plain objects (the engine takes
anything that carries the named attributes); the tables and the four functions below are the whole mechanism."""
import collections

import torch

# name: the attribute on the stage; tail: the shape behind [n_streams] - (), a constant, or the name of the stage's attribute that holds
# it; start: what a fresh or reset stream holds, None for a live parameter the caller fills and reset leaves alone
Field = collections.namedtuple("Field", ["name", "dtype", "tail", "start"])
_F32, _I32 = torch.float32, torch.int32

DOOR_STATE = (Field("in_state", _F32, "hist_in", 0.0), Field("out_state", _F32, "hist_out", 0.0))
DENOISE_STATE = (Field("reduction_db", _F32, (), None), Field("hist", _F32, "delay_size", 0.0), Field("ola", _F32, "delay_size", 0.0),
                 Field("smooth", _F32, 321, 0.0), Field("noise", _F32, 321, 0.0), Field("frames", _I32, (), 0), Field("noise_db", _F32, (), -200.0))
GATE_STATE = (Field("threshold_db", _F32, (), None), Field("open", _I32, (), 1), Field("hold", _I32, (), 0), Field("gain", _F32, (), 1.0),
              Field("level_db", _F32, (), -200.0))
TRACK_STATE = (Field("ring", _F32, "window_frames", 0.0), Field("count", torch.int64, (), 0), Field("auto", _F32, (), 0.0))
CARRY_STATE = (Field("scores", _F32, 512, 0.0),)      # the pitch path's best-predecessor values at the next window's first frame; zeros: a fresh path
SNAP_STATE = (Field("note", _I32, (), -1), Field("ratio", _F32, (), 1.0))      # the pitch correction's note and smoothed ratio at the next window's first frame; -1: no note
LOUDNESS_STATE = (Field("share", _F32, (), None), Field("src_ring", torch.float64, "window", 0.0), Field("out_ring", torch.float64, "window", 0.0),
                  Field("frames", torch.int64, (), 0), Field("gain", _F32, (), 1.0), Field("gain_db", _F32, (), 0.0))
LIMITER_STATE = (Field("ceiling", _F32, (), None), Field("tail", _F32, "sub_frame", 0.0), Field("peak", _F32, (), 0.0), Field("gain", _F32, (), 1.0),
                 Field("reduction_db", _F32, (), 0.0))


def _shape(stage, field, S):
    tail = field.tail
    return (S,) if tail == () else (S, getattr(stage, tail) if isinstance(tail, str) else tail)


def allocate(stage, table, device):
    """set every attribute of `table` on `stage` ([stage.n_streams, *tail] at its start value); live parameters are the caller's to fill"""
    for f in table:
        if f.start is not None:
            setattr(stage, f.name, torch.full(_shape(stage, f, stage.n_streams), f.start, dtype=f.dtype, device=device))


def reset(stage, table, streams=None):
    """Put every stream, or the listed ones, back at the start values.  In-place ops only: a captured graph reads these tensors when it
    replays, so they are never rebound."""
    idx = None if streams is None else torch.as_tensor(list(streams), dtype=torch.int64, device=getattr(stage, table[0].name).device)
    for f in table:
        if f.start is not None:
            t = getattr(stage, f.name)
            t.fill_(f.start) if idx is None else t.index_fill_(0, idx, f.start)


def checked(stage, table, S, device, what):
    """`stage`'s tensors in table order, each one on `device`, of the declared dtype, [S, *tail] and contiguous: the kernels index them by
    these shapes.  ValueError naming `what` + the field otherwise (what: "stream_gate: gate." and the like)."""
    out = []
    for f in table:
        t, shape = getattr(stage, f.name), _shape(stage, f, S)
        if not isinstance(t, torch.Tensor) or t.device != device:
            raise ValueError(f"{what}{f.name} must be a tensor on {device}, got {t.device if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dtype != f.dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}{f.name} must be contiguous {f.dtype} {list(shape)}, got {t.dtype} {tuple(t.shape)}")
        out.append(t)
    return out


def addresses(stage, table):
    """where the stage's tensors live, in table order: what a captured graph bakes in of them"""
    return tuple(getattr(stage, f.name).data_ptr() for f in table)
