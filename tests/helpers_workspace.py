"""A guarded, poisoned workspace for any Engine call, and guarded outputs (test_gpu_workspace_poison.py, test_gpu_stream_state.py; the helper
itself is proven on the host by test_workspace_guard_host.py).

Every library entry bump-allocates its scratch from the caller's workspace and hands regions back for later stages to reuse, so a stage that
reads a slot, a counter or a padded column it has not written this call finds the previous tenant's bytes.  Under the Engine's one grow-only
buffer those are usually the right values; for a caller who hands over fresh memory they are not.  The contract held here: an entry's outputs
are a function of its arguments alone, it writes nothing outside [ws, ws + ws_bytes) and its outputs, and it assumes nothing about the
workspace's contents or its position within a page.

guarded_workspace(eng, fill_word, phase) replaces eng._grow_ws on that instance for a `with` block.  Each request of `nbytes` is carved from an
arena [low guard | workspace | high guard]: the guards are 0xA5 bytes (the low one 65536 + 256 * phase of them, behind a 4 KiB-aligned start, so
the workspace base is 256-byte aligned at position 256 * phase of its page), the workspace is exactly nbytes - 4096 bytes - the measured peak:
every tvc_workspace_bytes* is the peak plus 4096 (api.h measure) - filled with the 32-bit `fill_word`.  Behind the block: a synchronize (the
decoder's side stream must have joined), then both guards of every arena byte for byte.
"""
import contextlib
import re

import numpy as np
import torch

GUARD_BYTE = 0xA5
WS_GUARD = 65536           # bytes of each workspace guard (the low one grows by 256 * phase)
OUT_GUARD = 4096           # bytes of each output guard
SLACK = 4096               # what every tvc_workspace_bytes* adds to the measured peak (api.h measure)
PAGE = 4096
# word        as fp32          as int32        as two fp16 / uint16     what it catches
# 0x00000000  0                0               0, 0                     the baseline in which a missing memset is invisible
# 0x7FC00000  quiet NaN        huge positive   NaN, 0                   any float read; sticks in an atomicMax done on the integer image
# 0xFFFFFFFF  NaN              -1              NaN, NaN / 65535         fp16 operands, back-pointers, counters; loses a signed integer max
# 0x7F7F7F7F  3.39e38, finite  huge positive   NaN, NaN                 a slot that is never zeroed keeps it: every scale changes, no NaN gives it away
FILLS = (0x00000000, 0x7FC00000, 0xFFFFFFFF, 0x7F7F7F7F)
PHASES = (0, 1, 5, 15)     # the phase that goes with each fill word in the GPU tests


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def fill_words(t, word):
    """t (uint8, 1-D) <- the 32-bit `word` repeated, little endian; a tail shorter than a word takes the word's first bytes"""
    n = t.numel() // 4
    if n:
        t[:4 * n].view(torch.int32).fill_(word - (1 << 32) if word >= 1 << 31 else word)
    for i in range(4 * n, t.numel()):
        t[i] = (word >> (8 * (i - 4 * n))) & 0xFF


def _changed(guard):
    """(first, last) offsets of the bytes of `guard` that are no longer GUARD_BYTE, or None"""
    bad = (guard != GUARD_BYTE).nonzero()
    return (int(bad[0]), int(bad[-1])) if bad.numel() else None


class _Arena:
    """[slack to a page | low guard | body | high guard] in one uint8 tensor; body = the workspace or an output"""

    def __init__(self, nbytes, low, high, device):
        self.nbytes, self.low, self.high = int(nbytes), int(low), int(high)
        self.raw = torch.empty(PAGE + self.low + self.nbytes + self.high, dtype=torch.uint8, device=device)
        self.start = -self.raw.data_ptr() % PAGE      # the low guard begins on a page
        self.raw.fill_(GUARD_BYTE)
        b = self.start + self.low
        self.body = self.raw[b:b + self.nbytes]

    def guards(self):
        b = self.start + self.low
        return self.raw[self.start:b], self.raw[b + self.nbytes:b + self.nbytes + self.high]

    def violations(self, what):
        """the guards' changed bytes in words: [] when both are intact"""
        lo, hi = self.guards()
        out = []
        c = _changed(lo)
        if c:      # offsets count back from the body's first byte
            out.append(f"{what}: the low guard changed from {what}_begin - {self.low - c[0]} to {what}_begin - {self.low - c[1]} "
                       f"(a store in front of the {self.nbytes} bytes)")
        c = _changed(hi)
        if c:
            out.append(f"{what}: the high guard changed from {what}_end + {c[0]} to {what}_end + {c[1]} (a store past the end of the {self.nbytes} bytes)")
        return out


class GuardedWorkspace:
    """what `with guarded_workspace(...) as g` yields: g.peaks = the bytes carved per request, g.arenas the arenas themselves"""

    def __init__(self):
        self.arenas = []

    @property
    def peaks(self):
        return [a.nbytes for a in self.arenas]

    def violations(self):
        return [v for a in self.arenas for v in a.violations("workspace")]


@contextlib.contextmanager
def _patched(eng, grow):
    """eng._grow_ws = grow on this instance for the block; the attribute and eng._ws are put back whatever happens inside"""
    had = "_grow_ws" in vars(eng)
    old_attr, old_ws = vars(eng).get("_grow_ws"), eng._ws
    eng._grow_ws = grow
    try:
        yield
    finally:
        if had:
            eng._grow_ws = old_attr
        else:
            del eng._grow_ws
        eng._ws = old_ws


@contextlib.contextmanager
def guarded_workspace(eng, fill_word, phase=0, peak=None, synchronize=None):
    """Every workspace an Engine method asks for inside the block is the measured peak of its query (nbytes - 4096; or `peak` bytes, for a
    stage call that borrows a conversion's query: exact_peak), filled with `fill_word`, between two guards.  Behind the block: `synchronize`
    (default: torch.cuda.synchronize on a GPU engine, nothing on a CPU one), then AssertionError if a guard byte changed, naming the first and
    last changed offset relative to the workspace's end (or its begin)."""
    if not 0 <= int(phase) < PAGE // 256:
        raise ValueError(f"phase must be in 0 .. {PAGE // 256 - 1}, got {phase!r}")
    g = GuardedWorkspace()

    def grow(nbytes):
        size = int(peak) if peak is not None else int(nbytes) - SLACK
        if size < 0:
            raise ValueError(f"a workspace query of {nbytes} bytes is below the {SLACK} every query adds to its peak")
        a = _Arena(size, WS_GUARD + 256 * int(phase), WS_GUARD, eng.device)
        fill_words(a.body, fill_word)
        g.arenas.append(a)
        eng._ws = a.body
        return a.body

    with _patched(eng, grow):
        yield g
    (synchronize if synchronize is not None else lambda: _sync(eng.device))()
    bad = g.violations()
    assert not bad, "; ".join(bad)


def exact_peak(eng, call):
    """The peak of a stage call that has no workspace query of its own (it borrows a conversion's: Engine._wsargs): `call()` runs once with
    a zero-byte workspace, is refused with TVC_ERR_WORKSPACE before anything launches (api.h run_walks), and the peak is read from the
    message's "need <peak> bytes".  None for a call that is not refused: it takes no workspace."""
    def grow(_nbytes):
        eng._ws = torch.empty(0, dtype=torch.uint8, device=eng.device)
        return eng._ws

    with _patched(eng, grow):
        try:
            call()
        except Exception as e:      # the engine's TinyVCError: "... failed (-4): workspace too small: need <peak> bytes, got 0"
            m = re.search(r"\(-4\).*need (\d+) bytes", str(e))
            if m is None:
                raise
            return int(m.group(1))
    return None


class GuardedOutput:
    """An output tensor that is a slice of its own guarded arena: .tensor for the call, .check() behind it (after a synchronize)"""

    def __init__(self, shape, dtype, fill, device="cpu"):
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        self.arena = _Arena(n, OUT_GUARD, OUT_GUARD, device)
        self.tensor = self.arena.body.view(dtype).view(*shape)
        self.tensor.fill_(fill)

    def violations(self):
        return self.arena.violations("output")

    def check(self):
        bad = self.violations()
        assert not bad, "; ".join(bad)


def guarded_output(shape, dtype, fill, device="cpu"):
    return GuardedOutput(shape, dtype, fill, device)


# ---- the comparison: bit pattern equality, NaN-safe (helpers_limiter.same_bits for tensors of any dtype) -------------------------------------
def _image(t):
    """the bytes of a tensor, on the host"""
    t = t.detach().contiguous().cpu()
    return t.reshape(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8)


def same_bits(a, b):
    """two tensors of one dtype and shape hold the same bit patterns, or NaN where the other holds NaN (floats).  Not torch.equal: that
    calls a tensor with a NaN different from itself."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if torch.equal(_image(a), _image(b)):
        return True
    if not a.dtype.is_floating_point:
        return False
    a, b = a.detach().cpu(), b.detach().cpu()
    size = a.element_size()
    ia, ib = (x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[size]) for x in (a, b))
    return bool(((ia == ib) | (a.isnan() & b.isnan())).all())


def first_difference(a, b):
    """where two tensors first differ in bits, in words, for a failure message"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    both_nan = (a.isnan() & b.isnan()) if a.dtype.is_floating_point else torch.zeros(a.shape, dtype=torch.bool)
    bytes_differ = (_image(a) != _image(b)).view(a.numel(), -1).any(dim=1)
    diff = (bytes_differ & ~both_nan).nonzero()
    if not diff.numel():
        return "no difference"
    i = int(diff[0])
    return f"{diff.numel()} of {a.numel()} elements differ, the first at flat index {i}: {a[i].item()!r} against {b[i].item()!r}"


def flatten(res):
    """every tensor of a result (a tensor, or nested tuples / lists of tensors and None), in order"""
    if isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, (tuple, list)):
        return [t for r in res for t in flatten(r)]
    return []


def assert_same_bits(got, want, what):
    got, want = flatten(got), flatten(want)
    assert len(got) == len(want), f"{what}: {len(got)} result tensors against {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"{what}: result tensor {i}: {first_difference(g, w)}"
