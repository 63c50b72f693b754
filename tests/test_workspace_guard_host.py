"""tests/helpers_workspace.py would fail a wrong kernel: proven on the host, with CPU tensors and a small fake engine whose "entries" write
and read where a wrong kernel would - the last workspace byte (legal), the first byte behind it, the byte in front of it, a workspace word this
call never wrote, the element behind an output.  No GPU and no library: the GPU files (test_gpu_workspace_poison.py, test_gpu_stream_state.py)
rest on exactly these properties of the helper."""
import pytest
import torch

import helpers_workspace as W


class FakeEngine:
    """what the helper touches of tinyvc_amd.engine.Engine: _grow_ws, _ws and a device; a `query` stands for a tvc_workspace_bytes* (peak + 4096)"""

    def __init__(self):
        self.device = torch.device("cpu")
        self._ws = None

    def _grow_ws(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8)
        return self._ws

    def entry(self, peak, body):
        """an Engine method: ask for the query's bytes, hand the workspace to the 'kernel'"""
        ws = self._grow_ws(peak + W.SLACK)
        assert ws is self._ws
        return body(ws)


def _raw_write(arena, offset_from_body, value=0):
    """a store at body[offset] that no slice bound stops: through the arena, as a kernel's pointer arithmetic would"""
    arena.raw[arena.start + arena.low + offset_from_body] = value


def test_the_last_workspace_byte_is_legal_and_the_bytes_around_it_are_not():
    eng = FakeEngine()
    with W.guarded_workspace(eng, 0x7FC00000) as g:
        eng.entry(1024, lambda ws: ws.__setitem__(-1, 0))
        eng.entry(1024, lambda ws: ws.__setitem__(0, 0))
    assert g.peaks == [1024, 1024]
    with pytest.raises(AssertionError, match=r"high guard changed from workspace_end \+ 0 to workspace_end \+ 0 "):
        with W.guarded_workspace(eng, 0) as g:
            eng.entry(1024, lambda ws: None)
            _raw_write(g.arenas[0], 1024)
    with pytest.raises(AssertionError, match=r"high guard changed from workspace_end \+ 256 to workspace_end \+ 65535 "):
        with W.guarded_workspace(eng, 0) as g:
            eng.entry(512, lambda ws: None)
            _raw_write(g.arenas[0], 512 + 256)
            _raw_write(g.arenas[0], 512 + 65535)
    with pytest.raises(AssertionError, match=r"low guard changed from workspace_begin - 1 to workspace_begin - 1 "):
        with W.guarded_workspace(eng, 0, phase=3) as g:
            eng.entry(1024, lambda ws: None)
            _raw_write(g.arenas[0], -1)
    with pytest.raises(AssertionError, match=r"workspace_begin - 66304 to workspace_begin - 2 .*workspace_end \+ 7 "):
        with W.guarded_workspace(eng, 0, phase=3) as g:      # the low guard's first byte (65536 + 256 * 3 in front) and both sides at once
            eng.entry(1024, lambda ws: None)
            _raw_write(g.arenas[0], -(65536 + 768))
            _raw_write(g.arenas[0], -2)
            _raw_write(g.arenas[0], 1024 + 7)
    # a store of the guard's own byte changes nothing that can be seen: the one thing the guards are blind to, by construction
    with W.guarded_workspace(eng, 0) as g:
        eng.entry(1024, lambda ws: None)
        _raw_write(g.arenas[0], 1024, W.GUARD_BYTE)


def test_the_second_request_of_a_block_is_checked_like_the_first():
    eng = FakeEngine()
    with pytest.raises(AssertionError, match=r"workspace_end \+ 3 "):
        with W.guarded_workspace(eng, 0) as g:
            eng.entry(256, lambda ws: None)
            eng.entry(768, lambda ws: None)
            _raw_write(g.arenas[1], 768 + 3)


@pytest.mark.parametrize("phase", range(16))
def test_the_slice_is_the_measured_peak_at_the_phase_of_its_page(phase):
    eng = FakeEngine()
    for nbytes in (W.SLACK + 256, W.SLACK + 256 * 37, W.SLACK + 4096 * 3):
        with W.guarded_workspace(eng, 0xFFFFFFFF, phase) as g:
            ws = eng._grow_ws(nbytes)
            assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() == nbytes - 4096 and eng._ws is ws
            assert ws.data_ptr() % 256 == 0 and ws.data_ptr() % 4096 == 256 * phase
            lo, hi = g.arenas[0].guards()
            assert lo.numel() == 65536 + 256 * phase and hi.numel() == 65536
            assert lo.data_ptr() + lo.numel() == ws.data_ptr() and ws.data_ptr() + ws.numel() == hi.data_ptr()
            assert bool((lo == 0xA5).all()) and bool((hi == 0xA5).all()) and bool((ws == 0xFF).all())
    with W.guarded_workspace(eng, 0, phase, peak=512) as g:      # a stage call's tight peak: whatever the borrowed query says
        assert eng._grow_ws(W.SLACK + 99999).numel() == 512 and g.peaks == [512]
    with W.guarded_workspace(eng, 0x7FC00000, phase, peak=0) as g:      # a call that takes no workspace: zero bytes between the guards
        assert eng._grow_ws(W.SLACK + 512).numel() == 0 and g.peaks == [0]
    with pytest.raises(ValueError):
        with W.guarded_workspace(eng, 0, 16):
            pass


@pytest.mark.parametrize("word", W.FILLS)
def test_the_fill_is_the_32_bit_word(word):
    eng = FakeEngine()
    with W.guarded_workspace(eng, word) as g:
        ws = eng._grow_ws(W.SLACK + 1024)
        assert [int(x) & 0xFFFFFFFF for x in ws.view(torch.int32).unique()] == [word]
        assert [int(b) for b in ws[:4]] == [(word >> s) & 0xFF for s in (0, 8, 16, 24)], "little endian, as the device reads it"
    odd = torch.zeros(11, dtype=torch.uint8)
    W.fill_words(odd, 0x04030201)
    assert odd.tolist() == [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3]


def test_a_result_that_reads_an_unwritten_word_differs_under_the_fills_and_the_comparison_says_so():
    """the GPU tests' scheme end to end: `want` from the engine's own workspace, then the same call under every fill word.  The sound entry
    writes its slot before it reads it; the wrong one adds an atomicMax-style slot it never zeroed (what the previous call left is exactly
    right under the grow-only buffer: the ordinary engine cannot see it)."""
    eng = FakeEngine()
    x = torch.tensor([0.5, -2.0, 1.25])

    def sound(ws):
        slot = ws[256:260].view(torch.float32)
        slot[0] = 0.0                                   # "zeroed here"
        slot[0] = torch.maximum(slot[0], x.abs().max())
        return x / slot[0], slot.view(torch.int32).clone()

    def wrong(ws):
        slot = ws[256:260].view(torch.int32)            # the maximum on the integer image, no memset in front of it
        slot[0] = torch.maximum(slot[0], x.abs().max().view(torch.int32))
        return x / slot.view(torch.float32)[0], slot.clone()

    def reads(ws):                                      # a padded column nobody wrote, added in: every fill but the baseline shows
        return x + ws[512:516].view(torch.float32)[0], x.clone()

    eng._grow_ws(W.SLACK + 1024).zero_()                # the engine's own buffer as the first call of a process finds it here
    for entry, differing in ((sound, []), (wrong, [0x7FC00000, 0x7F7F7F7F]), (reads, [0x7FC00000, 0xFFFFFFFF, 0x7F7F7F7F])):
        want = eng.entry(1024, entry)
        assert W.same_bits(eng.entry(1024, entry)[0], want[0]), "self-healing under the grow-only buffer: the second call of the same shape"
        seen = []
        for word, phase in zip(W.FILLS, W.PHASES):
            with W.guarded_workspace(eng, word, phase):
                got = eng.entry(1024, entry)
            try:
                W.assert_same_bits(got, want, f"fill {word:#010x}")
            except AssertionError as e:
                assert "result tensor 0" in str(e) and "elements differ, the first at flat index 0" in str(e)
                seen.append(word)
        # 0 is the baseline that hides it; 0xFFFFFFFF is -1 as an integer and loses the signed max (the table in helpers_workspace.py)
        assert seen == differing, (entry.__name__, [hex(w) for w in seen])


def test_the_comparison_is_bit_equality_that_lets_a_nan_equal_a_nan():
    nan, a = float("nan"), torch.tensor([1.0, float("nan"), -0.0])
    assert not torch.equal(a, a.clone()), "torch.equal is not the comparison: a NaN differs from itself"
    assert W.same_bits(a, a.clone())
    assert not W.same_bits(a, torch.tensor([1.0, nan, 0.0])), "-0.0 and 0.0 are different bits"
    assert not W.same_bits(a, torch.tensor([1.0, 2.0, -0.0])) and not W.same_bits(torch.tensor([1.0, 2.0, -0.0]), a)
    assert W.same_bits(torch.tensor([nan]), torch.tensor([0x7F7F7F7F | 0x00800000], dtype=torch.int32).view(torch.float32)), "any NaN for any NaN"
    assert not W.same_bits(a, a.double()) and not W.same_bits(a, a[:2])
    i = torch.tensor([3, -1, 7], dtype=torch.int64)
    assert W.same_bits(i, i.clone()) and not W.same_bits(i, torch.tensor([3, -1, 8], dtype=torch.int64))
    assert W.same_bits(torch.empty(0), torch.empty(0))
    assert "1 of 3 elements differ, the first at flat index 2" in W.first_difference(i, torch.tensor([3, -1, 8], dtype=torch.int64))
    W.assert_same_bits((a, None, [i]), (a.clone(), None, [i.clone()]), "nested results")
    with pytest.raises(AssertionError, match="result tensor 1"):
        W.assert_same_bits((a, i), (a, i + 1), "the second tensor")
    with pytest.raises(AssertionError, match="2 result tensors against 1"):
        W.assert_same_bits((a, i), (a,), "a missing tensor")


def test_the_patch_and_the_workspace_are_restored_after_an_exception():
    eng = FakeEngine()
    own = eng._grow_ws(4096 + 512)
    assert "_grow_ws" not in vars(eng)
    with pytest.raises(RuntimeError, match="inside"):
        with W.guarded_workspace(eng, 0x7F7F7F7F, 5):
            assert "_grow_ws" in vars(eng) and eng._grow_ws(4096 + 512) is not own and eng._ws is not own
            raise RuntimeError("inside")
    assert "_grow_ws" not in vars(eng) and eng._ws is own and eng._grow_ws(16) is own, "the class's method again, and the buffer it grew"
    with W.guarded_workspace(eng, 0):      # ... and after a clean block
        eng._grow_ws(4096 + 256)
    assert "_grow_ws" not in vars(eng) and eng._ws is own
    with pytest.raises(AssertionError):      # ... and after a block whose guard check fails
        with W.guarded_workspace(eng, 0) as g:
            eng._grow_ws(4096 + 256)
            _raw_write(g.arenas[0], 256)
    assert "_grow_ws" not in vars(eng) and eng._ws is own
    other = FakeEngine()      # this instance only
    with W.guarded_workspace(eng, 0):
        assert "_grow_ws" not in vars(other) and other._grow_ws(64).numel() == 64
    marker = eng._grow_ws
    eng._grow_ws = marker      # an instance that already carries an attribute of its own gets that one back
    with W.guarded_workspace(eng, 0):
        pass
    assert vars(eng)["_grow_ws"] == marker


def test_the_synchronize_runs_behind_the_block_and_in_front_of_the_check():
    eng, order = FakeEngine(), []
    with pytest.raises(AssertionError, match="high guard"):
        with W.guarded_workspace(eng, 0, synchronize=lambda: (order.append("sync"), _raw_write(g.arenas[0], 256))) as g:
            eng._grow_ws(4096 + 256)      # a store that lands only when the side stream is waited for
            order.append("block")
    assert order == ["block", "sync"]


def test_exact_peak_reads_the_refusal_of_a_zero_byte_workspace():
    eng = FakeEngine()
    own = eng._grow_ws(8192)

    def refused():
        ws = eng._grow_ws(4096 + 99999)
        assert ws.numel() == 0 and eng._ws is ws
        raise RuntimeError("tvc_encoder_f32 failed (-4): workspace too small: need 70400 bytes, got 0")

    assert W.exact_peak(eng, refused) == 70400
    assert "_grow_ws" not in vars(eng) and eng._ws is own
    assert W.exact_peak(eng, lambda: None) is None, "a call that is not refused takes no workspace"

    def other():
        raise RuntimeError("tvc_encoder_f32 failed (-2): bad argument")
    with pytest.raises(RuntimeError, match="bad argument"):
        W.exact_peak(eng, other)
    assert "_grow_ws" not in vars(eng) and eng._ws is own


@pytest.mark.parametrize("shape, dtype, fill", [((2, 17760), torch.float32, float("nan")), ((2, 37, 4), torch.int64, -7), ((3,), torch.float16, 1.0),
                                                  ((37,), torch.int32, -7), ((5, 3), torch.uint8, 9)])
def test_a_guarded_output_sees_a_store_one_element_behind_the_tensor(shape, dtype, fill):
    out = W.guarded_output(shape, dtype, fill)
    t = out.tensor
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 4096 == 0
    assert bool((t != t).all()) if fill != fill else bool((t == fill).all())
    t.reshape(-1)[-1] = 0      # the last element is the tensor's
    t.reshape(-1)[0] = 0
    out.check()
    size, n = t.element_size(), t.numel()
    for k in range(size):      # one element behind it
        _raw_write(out.arena, n * size + k)
    with pytest.raises(AssertionError, match=rf"high guard changed from output_end \+ 0 to output_end \+ {size - 1} "):
        out.check()
    front = W.guarded_output(shape, dtype, fill)
    _raw_write(front.arena, -1)
    with pytest.raises(AssertionError, match=r"low guard changed from output_begin - 1 to output_begin - 1 "):
        front.check()
