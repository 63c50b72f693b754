"""The per-stream pitch tracker on the device (tvc_pitch_track_f32, tvc_convert_track_f32; feature_retrieval.PitchTrack,
Generator.convert(track=...), BatchedStreamInfer(auto_pitch=...), infer_streaming.py --auto-pitch).

The stage call runs on synthetic f0, without a model, against the CPU model of tests/test_pitch_track_host.py (a Python list per stream,
torch.median, a ring filled one value at a time): the ring slot by slot, the count and the median's bits after EVERY call; streams of one
launch do not see each other nor the columns outside the tracked ones; the shift is the fp64 formula rounded once (bit for bit
tvc_pitch_match_f32's where both apply), ramps exactly under a power-of-two slew and lands on the wanted value itself.  End to end a tracked
stream block equals, bit for bit, the untracked block fed the shifts it reports; a captured graph equals eager and survives a reset, new
target registers and the history advancing without a new capture."""
import math

import numpy as np
import pytest
import torch

from helpers import state_dicts
from test_gpu_auto_pitch import _row, _spread, _ulps
from test_pitch_track_host import TrackModel
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1500, 8192]      # around a wave and the workgroup's pass; the default; the cap
NEW = [0, 1, 4, 63, 64, 65, 256]                                      # around a wave and the workgroup
PATTERNS = ["unvoiced_blocks", "one_voiced", "all_equal", "last_bits", "exponents", "nan_negative"]
HEAD, TAIL = 2, 3                                                      # poisoned columns in front of and behind the tracked ones
POISON = 1e30


def _engine():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _track(S, n, W, min_voiced=1, slew=math.inf):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    return PitchTrack(S, n, lag_frames=TAIL, window_frames=W, min_voiced=min_voiced, slew=slew, device=DEV)


def _f0(cols):
    """[S, n] new frames -> f0 [S, HEAD + n + TAIL] with poison everywhere else: it must never enter a ring"""
    S, n = cols.shape
    f0 = torch.full((S, HEAD + n + TAIL), POISON)
    f0[:, HEAD:HEAD + n] = cols
    return f0.to(DEV)


def _block(pattern, n, call, seed):
    """the n new frames of call number `call` of a stream that follows `pattern` (tests/test_gpu_auto_pitch.py's value patterns)"""
    if n == 0:
        return torch.zeros(0)
    if pattern == "unvoiced_blocks":      # every other block has no voiced frame at all
        return torch.zeros(n) if call % 2 == 0 else _spread(n, torch.Generator().manual_seed(seed))
    if pattern == "one_voiced":           # one voiced frame per block, wandering through the block (and so through every wave)
        x = torch.zeros(n)
        x[(7 * call) % n] = 100.0 + call
        return x
    return _row(pattern, n, seed)


def _bits(x):
    return torch.as_tensor(x).cpu().contiguous().view(torch.int32)


def _check_state(tag, eng, tr, model, med, cnt):
    """everything the device holds after a call against the model: ring (multiset and slot by slot), count, the median's bits; and against
    tvc_pitch_match_f32 over the ring rows (the same select, from global memory): its median and its voiced count = the fill"""
    ring = tr.ring.cpu()
    want = torch.from_numpy(model.ring)
    assert torch.equal(ring.sort(dim=1).values, want.sort(dim=1).values), f"{tag}: the ring holds other values than the last W voiced ones"
    assert torch.equal(_bits(ring), _bits(want)), f"{tag}: the ring's slots are not those of a one-by-one append"
    assert tr.count.cpu().tolist() == model.count.tolist() and cnt.cpu().tolist() == model.count.tolist(), f"{tag}: count {tr.count.tolist()} != {model.count.tolist()}"
    assert torch.equal(_bits(med), _bits(model.med)), f"{tag}: median {med.tolist()} != torch.median {model.med.tolist()}"
    m2, v2, _sh, _ = eng.pitch_match(tr.ring)
    fill = np.minimum(model.count, model.W)
    assert torch.equal(_bits(m2), _bits(med)) and v2.cpu().tolist() == fill.tolist(), f"{tag}: pitch_match over the ring rows disagrees"


@pytest.mark.parametrize("W", WINDOWS)
def test_ring_and_select_bit_for_bit(W):
    eng = _engine()
    S = len(PATTERNS)
    target = torch.full((S,), 200.0, device=DEV)
    wrapped = 0
    for n in NEW:
        calls = min(40, max(6, -(-5 * W // (2 * max(n, 1))) + 1))      # 2.5 windows of a fully voiced block, within 6 .. 40 calls
        tr, model = _track(S, n, W), TrackModel(S, W)
        for c in range(calls):
            cols = torch.stack([_block(p, n, c, 1000 * W + 10 * c + i) for i, p in enumerate(PATTERNS)])
            med, cnt, _sh, _ = eng.pitch_track(_f0(cols), tr, target)
            model.med, _ = model.step(cols.numpy(), [200.0] * S, [0.0] * S)
            _check_state(f"W = {W}, n = {n}, call {c}", eng, tr, model, med, cnt)
        assert n == 0 or model.count[PATTERNS.index("all_equal")] == n * calls
        assert model.count[PATTERNS.index("one_voiced")] == (calls if n else 0)
        wrapped = max(wrapped, int(model.count[2:].min()) // W)      # the four streams that are voiced in most frames of every block
    assert W > 257 or wrapped >= 2, f"W = {W}: no case wrapped the dense streams' rings twice"


@pytest.mark.parametrize("W", [1, 2, 3])
def test_more_voiced_frames_than_the_ring_holds(W):
    """nv > W in one block (n = 4, all voiced): the last W survive, in the slots a one-by-one append leaves them in"""
    eng = _engine()
    tr, model = _track(1, 4, W), TrackModel(1, W)
    for c in range(6):
        cols = torch.tensor([[10.0 + 4 * c + k for k in range(4)]])
        med, cnt, _sh, _ = eng.pitch_track(_f0(cols), tr, torch.tensor([100.0], device=DEV))
        model.med, _ = model.step(cols.numpy(), [100.0], [0.0])
        _check_state(f"W = {W}, call {c}", eng, tr, model, med, cnt)
        assert sorted(tr.ring[0].tolist()) == cols[0, 4 - W:].tolist() and int(cnt[0]) == 4 * (c + 1)


def test_neighbours_and_poison():
    """S = 5 streams of different histories in one launch (one never voiced), poison outside the tracked columns: every stream equals its
    own S = 1 run, state and outputs, call after call."""
    eng = _engine()
    S, n, W = 5, 65, 64
    g = torch.Generator().manual_seed(5)
    target = torch.tensor([300.0, 150.0, 220.0, 97.3, 440.0], device=DEV)
    offs = [0.0, 1.0, -2.0, 3.0, 0.25]
    both = _track(S, n, W, min_voiced=3)
    alone = [_track(1, n, W, min_voiced=3) for _ in range(S)]
    for c in range(5):
        cols = torch.stack([_spread(n, g) * (1.0 + 0.2 * s) for s in range(S)])
        cols[1][torch.rand(n, generator=g) < 0.5] = 0.0
        cols[2] = -cols[2]                                       # never voiced, between voiced ones
        cols[3][torch.rand(n, generator=g) < 0.97] = float("nan")     # a frame or two per block: warms up late
        f0 = _f0(cols)
        med, cnt, sh, f0s = eng.pitch_track(f0, both, target, offs, want_shifted=True)
        for s in range(S):
            m1, c1, s1, f1 = eng.pitch_track(f0[s:s + 1].contiguous(), alone[s], target[s:s + 1].contiguous(), offs[s], want_shifted=True)
            tag = f"call {c}, stream {s}: its neighbours leaked into it"
            assert torch.equal(_bits(med[s:s + 1]), _bits(m1)) and torch.equal(cnt[s:s + 1], c1) and torch.equal(_bits(sh[s:s + 1]), _bits(s1)), tag
            assert torch.equal(_bits(f0s[s:s + 1]), _bits(f1)), tag
            assert torch.equal(_bits(both.ring[s]), _bits(alone[s].ring[0])) and torch.equal(both.auto[s:s + 1], alone[s].auto), tag
        assert float(both.ring.max()) < 1e29, "poison from outside the tracked columns entered a ring"
    assert int(both.count[2]) == 0 and float(med[2]) == 0.0 and float(sh[2]) == offs[2] and not both.ring[2].any()
    assert int(both.count[0]) == 5 * n and 0 < int(both.count[3]) < int(both.count[1]) < 5 * n


def test_shift_is_the_offset_without_a_register():
    """Before warm-up (fill < min_voiced), with a target <= 0 or NaN, and for a stream without a voiced frame: auto == 0 and shift == offset
    exactly; then warm-up is crossed."""
    eng = _engine()
    S, n = 4, 4
    tr = _track(S, n, 32, min_voiced=10)
    target = torch.tensor([220.0, 0.0, float("nan"), -50.0], device=DEV)
    offs = [1.25, -0.75, 3.0, 0.1]
    cols = torch.full((S, n), 110.0)
    for c in range(4):
        _m, cnt, sh, _ = eng.pitch_track(_f0(cols), tr, target, offs)
        if c < 2:      # 4 and 8 values in the ring: below min_voiced = 10
            assert tr.auto.tolist() == [0.0] * S and sh.tolist() == [np.float32(o).item() for o in offs], f"call {c}: {sh.tolist()}"
    assert tr.auto.tolist() == [12.0, 0.0, 0.0, 0.0] and sh.tolist() == [13.25] + [np.float32(o).item() for o in offs[1:]] and cnt.tolist() == [16] * S


def test_shift_is_pitch_match_s_and_the_fp64_formula():
    """Offset 0, slew = inf, min_voiced = 1, fresh state: shift_out == tvc_pitch_match_f32's shift over the same columns BIT FOR BIT (the same
    fp64 expression rounded once; 0.0 + x is exact).  With other offsets: within 1 fp32 ulp of numpy's fp64 evaluation (the margin
    tests/test_gpu_auto_pitch.py gives two fp64 evaluations of one formula)."""
    eng = _engine()
    S, n = 8, 63
    g = torch.Generator().manual_seed(11)
    cols = torch.stack([_spread(n, g) for _ in range(S)])
    cols[torch.rand(S, n, generator=g) < 0.2] = 0.0
    target = torch.exp(torch.empty(S).uniform_(float(np.log(60.0)), float(np.log(900.0)), generator=g)).to(DEV)
    f0 = _f0(cols)
    med, _cnt, sh, _ = eng.pitch_track(f0, _track(S, n, 256), target)
    T = f0.shape[1]
    starts = sorted([s * T + HEAD for s in range(S)] + [s * T + HEAD + n for s in range(S)])      # the tracked columns and the poison between them, as rows
    m2, _v2, s2, _ = eng.pitch_match(f0, starts + [starts[-1]], torch.stack([target, target], 1).reshape(-1).contiguous())
    assert torch.equal(_bits(med), _bits(m2[0::2])) and torch.equal(_bits(sh), _bits(s2[0::2])), f"{sh.tolist()} != pitch_match's {s2[0::2].tolist()}"
    assert len(set(sh.tolist())) == S
    # The offsets take the sign of the automatic shift: shift = fl(offset + fl(auto)) is then within half an ulp of `auto` plus half an ulp of
    # the (larger) sum of offset + auto in fp64, i.e. within 1 ulp of it.  (Against an offset of the other sign the sum is smaller than the
    # automatic part, whose own rounding then weighs more than an ulp of the sum: the fp32 add of step 6 is the definition, and the second
    # check below holds it for either sign.)
    mags = [0.5, 1.0, 2.0, 7.0, 12.0, 0.125, 24.0, 0.3]
    for sign in (1.0, -1.0):
        offs = [float(np.copysign(m, sign * float(a))) for m, a in zip(mags, sh)]
        _m, _c, sh3, _ = eng.pitch_track(f0, _track(S, n, 256), target, offs)
        for s in range(S):
            exact = np.float64(np.float32(offs[s])) + 12.0 * np.log2(np.float64(target[s].item()) / np.float64(med[s].item()))
            d = int(_ulps(sh3[s:s + 1].cpu(), torch.tensor([np.float32(exact)]))[0])
            print(f"[pitch track] stream {s}: offset {offs[s]:+}, shift {float(sh3[s])!r}, numpy fp64 {float(np.float32(exact))!r}: {d} ulp")
            if sign > 0:
                assert d <= 1, f"stream {s}: {d} ulps from the fp64 formula"
            assert float(sh3[s]) == np.float32(np.float32(offs[s]) + np.float32(sh[s].item())), f"stream {s}: the shift is not ONE fp32 add of the offset and the automatic part"


@pytest.mark.parametrize("direction", [1, -1])
def test_slew_ramps_exactly_and_lands(direction):
    """slew = 0.25 (a power of two: every step of the ramp is exact), the target an octave (and, second stream, 5.37 semitones) away from the
    history: auto goes 0.25, 0.5, ... and then lands on `wanted` bit for bit; slew = 0 never moves."""
    eng = _engine()
    hist = [110.0, 110.0] if direction > 0 else [220.0, 150.0]
    target = torch.tensor([220.0, 150.0] if direction > 0 else [110.0, 110.0], device=DEV)
    cols = torch.tensor([[hist[0]] * 4, [hist[1]] * 4])
    tr, still = _track(2, 4, 16, slew=0.25), _track(2, 4, 16, slew=0.0)
    free = _track(2, 4, 16)
    eng.pitch_track(_f0(cols), free, target)
    wanted = free.auto.clone()      # slew = inf: lands at once
    assert abs(float(wanted[0])) == 12.0 and 5.3 < abs(float(wanted[1])) < 5.4
    for k in range(1, 52):
        _m, _c, sh, _ = eng.pitch_track(_f0(cols), tr, target, 1.0)
        eng.pitch_track(_f0(cols), still, target, 1.0)
        want = [direction * 0.25 * k if 0.25 * k < abs(float(w)) else float(w) for w in wanted]
        assert tr.auto.tolist() == want, f"step {k}: auto {tr.auto.tolist()}, the exact ramp gives {want}"
        assert sh.tolist() == [np.float32(1.0 + a).item() for a in want]
        assert still.auto.tolist() == [0.0, 0.0]
    assert torch.equal(_bits(tr.auto), _bits(wanted)), "the ramp did not land on the wanted shift itself"


def test_f0_shifted_is_shift_frequency():
    eng = _engine()
    S, n = 3, 64
    g = torch.Generator().manual_seed(21)
    cols = torch.stack([_spread(n, g) for _ in range(S)])
    f0 = _f0(cols)
    f0[:, :HEAD] = 0.0
    f0[:, -TAIL:] = torch.tensor([55.0, 0.0, 880.0])      # all T columns are shifted, the untracked ones too
    _m, _c, sh, f0s = eng.pitch_track(f0, _track(S, n, 128), torch.tensor([220.0, 110.0, 330.0], device=DEV), [0.0, 0.5, -0.5], want_shifted=True)
    assert len(set(sh.tolist())) == S
    for s in range(S):
        assert torch.equal(_bits(f0s[s]), _bits(eng.shift_frequency(f0[s], float(sh[s])))), f"stream {s}"
    # a launch over the middle stream alone writes that stream's columns only
    canvas = torch.full((S, f0.shape[1]), -7.0, device=DEV)
    tr = _track(1, n, 128)
    targs = eng._track_args(tr, 1, f0.shape[1])
    import ctypes
    one = torch.tensor([110.0], device=DEV)
    rc = eng.lib.tvc_pitch_track_f32(eng.ctx, eng._stream(), ctypes.c_void_p(f0[1].data_ptr()), 1, f0.shape[1], targs[0], targs[1],
                                     ctypes.c_void_p(one.data_ptr()), 0.5, None, *targs[2:], None, None, None,
                                     ctypes.c_void_p(canvas[1].data_ptr()))
    assert rc == 0
    assert torch.equal(_bits(canvas[1]), _bits(f0s[1])) and bool((canvas[0] == -7.0).all()) and bool((canvas[2] == -7.0).all()), "columns of other streams were written"


def test_reset_restarts_the_listed_streams_only():
    eng = _engine()
    S, n, W = 3, 4, 8
    g = torch.Generator().manual_seed(31)
    target = torch.tensor([220.0, 110.0, 330.0], device=DEV)
    tr, model = _track(S, n, W, min_voiced=5, slew=0.5), TrackModel(S, W, min_voiced=5, slew=0.5)
    for c in range(8):
        if c == 4:
            tr.reset([1])
            model.reset([1])
            assert not tr.ring[1].any() and int(tr.count[1]) == 0 and float(tr.auto[1]) == 0.0 and tr.count.tolist()[0] == 16
        cols = torch.empty(S, n).uniform_(120.0, 180.0, generator=g)      # between the targets: every stream's ramp keeps its direction
        med, cnt, sh, _ = eng.pitch_track(_f0(cols), tr, target)
        model.med, msh = model.step(cols.numpy(), target.tolist(), [0.0] * S)
        _check_state(f"call {c}", eng, tr, model, med, cnt)
        if c == 4:
            assert float(sh[1]) == 0.0 and float(sh[0]) != 0.0 and float(sh[2]) != 0.0, "stream 1 warms up again, the others go on"
        assert int(_ulps(sh.cpu(), torch.from_numpy(msh)).max()) <= 1
        model.auto[:] = tr.auto.cpu().numpy()      # (a landed value may sit one ulp from numpy's: do not let that compound)
    assert tr.count.tolist() == [32, 16, 32]


def test_the_entry_refuses_bad_arguments():
    from tinyvc_amd._lib import TinyVCError
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    eng = _engine()
    f0, f0big = torch.zeros(2, 28, device=DEV), torch.zeros(2, 300, device=DEV)
    tgt = torch.ones(2, device=DEV)
    with pytest.raises(ValueError, match="do not fit"):
        eng.pitch_track(f0, PitchTrack(2, 4, lag_frames=25, device=DEV), tgt)
    with pytest.raises(ValueError, match="a tracker of 3 streams"):
        eng.pitch_track(f0, PitchTrack(3, 4, device=DEV), tgt)
    tr = PitchTrack(2, 4, device=DEV)
    tr.window_frames = 8192      # a tracker whose tensors no longer have the shape its parameters say: refused on the host
    with pytest.raises(ValueError, match="track.ring"):
        eng.pitch_track(f0, tr, tgt)
    tr.window_frames = 1500
    # past the Python checks: the library checks every host value itself, before any device work
    import ctypes
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(T=28, start=24, n=4, W=1500, min_voiced=1, slew=0.0, f0_=f0, target=tgt):
        x = f0big if T == 300 else f0_
        rc = eng.lib.tvc_pitch_track_f32(eng.ctx, eng._stream(), ptr(x) if x is not None else None, 2, T, start, n, ptr(target) if target is not None else None,
                                         0.0, None, W, min_voiced, slew, ptr(tr.ring), ptr(tr.count), ptr(tr.auto), None, None, None, None)
        return rc, eng.lib.tvc_last_error(eng.ctx).decode()
    assert call()[0] == 0
    for kw, what in ((dict(W=8193), "W = 8193"), (dict(W=0), "W = 0"), (dict(T=300, start=0, n=257), "n = 257"), (dict(n=-1), "n = -1"), (dict(min_voiced=0), "min_voiced"),
                     (dict(slew=-1.0), "slew"), (dict(slew=float("nan")), "slew"), (dict(start=25), "do not lie within T = 28"), (dict(start=-1), "do not lie within"),
                     (dict(f0_=None), "f0 is NULL"), (dict(target=None), "target_f0 is NULL")):
        rc, msg = call(**kw)
        assert rc != 0 and what in msg, (kw, rc, msg)
    with pytest.raises(TinyVCError):
        eng._ok(call(W=0)[0], "tvc_pitch_track_f32")
    torch.cuda.synchronize()
    assert not tr.ring.any() and not tr.count.any(), "a refused call (or the all-unvoiced one) touched the state"


# ---- end to end: streams ---------------------------------------------------------------------------------------------------------------------
REGISTERS = [220.0, 110.0, 330.0]
OFFSETS = [0.5, -1.0, 0.25]
N_BLOCKS = 12


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.fixture(scope="module")
def stream_inputs():
    blocks = synth.synth_wave(3, N_BLOCKS * 1920, seed=50).view(3, N_BLOCKS, 1920).to(DEV)
    tgt = synth.synth_index(500, seed=2).to(DEV)
    angles = [synth.synth_angle(3, 28, 700 + i).to(DEV) for i in range(N_BLOCKS)]
    return blocks, tgt, angles


def _stream(gen, tgt, track_kw=None, registers=None, use_graph=False, pitch_shift=OFFSETS):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    track = PitchTrack(3, 4, lag_frames=8, device=DEV, **track_kw) if track_kw is not None else None
    st = BatchedStreamInfer(gen, n_streams=3, target=tgt, pitch_shift=pitch_shift, device=torch.device(DEV), block_size=1920, extra_size=3840,
                            use_graph=use_graph, auto_pitch=registers, pitch_track=track)
    st.init_buffer()
    assert st.input_size // 480 == 28 and (track is None or track.columns(28) == (16, 4))
    return st


@pytest.mark.parametrize("track_kw", [dict(min_voiced=10), dict(min_voiced=10, window_frames=16, slew=0.25)], ids=["default_window", "evicting_and_ramping"])
def test_stream_blocks_equal_the_untracked_stream_fed_their_shifts(gen, stream_inputs, track_kw):
    """Per block, eager: the tracked stream's output == the untracked BatchedStreamInfer's, bit for bit, fed last_pitch_shift of that block as
    host per-stream shifts; the shift == the CPU model fed the values that entered the ring (read back from the device ring via count),
    exactly while it is the offset or on the ramp, within 1 ulp where it landed on the fp64 formula."""
    blocks, tgt, angles = stream_inputs
    W, slew = track_kw.get("window_frames", 1500), track_kw.get("slew", math.inf)
    st = _stream(gen, tgt, track_kw, torch.tensor(REGISTERS, device=DEV))
    plain = _stream(gen, tgt)
    model = TrackModel(3, W, min_voiced=10, slew=slew)
    per_block, seen = [], []
    for i in range(N_BLOCKS):
        before = st.pitch_track.count.cpu().numpy().copy()
        out = st.audio_callback(blocks[:, i], noise_angle=angles[i]).clone()
        sh = st.last_pitch_shift.cpu()
        plain.pitch_shift = sh.tolist()
        want = plain.audio_callback(blocks[:, i], noise_angle=angles[i])
        assert torch.equal(st.last_shift, plain.last_shift), f"block {i}: SOLA lags differ"
        assert torch.equal(out, want), f"block {i}: the tracked stream != the untracked stream fed its shifts {sh.tolist()}"
        after, ring = st.pitch_track.count.cpu().numpy(), st.pitch_track.ring.cpu().numpy()
        new = [[ring[s, (before[s] + j) % W] for j in range(after[s] - before[s])] for s in range(3)]
        per_block.append([len(x) for x in new])
        assert all(0 <= len(x) <= 4 and all(v > 0 for v in x) for x in new)
        _med, msh = model.step(new, REGISTERS, OFFSETS)
        assert torch.equal(torch.from_numpy(model.ring), st.pitch_track.ring.cpu()) and model.count.tolist() == after.tolist()
        print(f"[pitch track] block {i}: voiced {per_block[-1]}, medians {_med.tolist()}, shifts {sh.tolist()} (model {msh.tolist()})")
        for s in range(3):
            landed = model.auto[s] == model.wanted[s] and model.wanted[s] != 0
            d = int(_ulps(sh[s:s + 1], torch.tensor([msh[s]]))[0])
            assert d <= (1 if landed else 0), f"block {i}, stream {s}: shift {float(sh[s])!r}, the model {float(msh[s])!r} ({'landed' if landed else 'offset / ramp'})"
        assert torch.equal(sh, torch.tensor(OFFSETS) + st.pitch_track.auto.cpu()), "the shift is not one fp32 add of the offset and `auto`"
        model.auto[:] = st.pitch_track.auto.cpu().numpy()      # a landed value may sit one ulp from numpy's: do not let that compound
        seen.append(sh.tolist())
    # not vacuous: every stream heard voiced frames, crossed warm-up, and the streams' shifts differ pairwise
    assert all(c > 10 for c in model.count) and len(set(seen[-1])) == 3 and seen[0] == [np.float32(o).item() for o in OFFSETS]
    assert all(abs(a - o) > 0.2 for a, o in zip(seen[-1], OFFSETS)), f"no automatic shift was applied: {seen[-1]}"
    if W == 16:
        assert all(c > W for c in model.count), "the ring did not evict"
        assert any(abs(abs(seen[k][s] - OFFSETS[s]) - 0.25) < 1e-6 for k in range(N_BLOCKS) for s in range(3)), "no ramp step was seen"


def _run(gen, stream_inputs, use_graph, events=False):
    blocks, tgt, angles = stream_inputs
    registers = torch.tensor(REGISTERS, device=DEV)
    st = _stream(gen, tgt, dict(min_voiced=10), registers, use_graph)
    outs, lags, shifts, graphs = [], [], [], []
    for i in range(N_BLOCKS):
        if events and i == 5:
            st.pitch_track.reset([0])
        if events and i == 6:
            registers.copy_(torch.tensor([150.0, 260.0, 95.0], device=DEV))
        outs.append(st.audio_callback(blocks[:, i], noise_angle=angles[i]).clone())
        lags.append(st.last_shift.clone())
        shifts.append(st.last_pitch_shift.clone())
        graphs.append(st._graph[1][True][0] if use_graph and st._graph is not None and True in st._graph[1] else None)
    tr = st.pitch_track
    return torch.stack(outs), torch.stack(lags), torch.stack(shifts), (tr.ring.clone(), tr.count.clone(), tr.auto.clone()), graphs, st


def test_stream_graph_replay_equals_eager(gen, stream_inputs):
    eager = _run(gen, stream_inputs, False)
    graph = _run(gen, stream_inputs, True)
    assert graph[5]._graph is not None and graph[5]._graph[1], "blocks 3.. must have replayed the captured graph"
    assert torch.equal(eager[1], graph[1]), "SOLA lags differ between eager and graph replay"
    assert torch.equal(eager[2], graph[2]), f"last_pitch_shift differs: {eager[2].tolist()} / {graph[2].tolist()}"
    assert torch.equal(eager[0], graph[0]), "graph replay is not sample-exact"
    for a, b, name in zip(eager[3], graph[3], ("ring", "count", "auto")):
        assert torch.equal(a, b), f"the final {name} differs"
    assert bool((eager[3][1] > 10).all()) and len(set(eager[2][-1].tolist())) == 3


def test_stream_graph_survives_reset_and_new_registers(gen, stream_inputs):
    """track.reset([0]) before block 5 and registers.copy_(...) before block 6, and the history advancing all along: the graph captured at
    block 2 replays to the end (the same graph object) and still equals eager."""
    eager = _run(gen, stream_inputs, False, events=True)
    graph = _run(gen, stream_inputs, True, events=True)
    g = graph[4]
    assert g[2] is not None and all(x is g[2] for x in g[2:]), "a reset / new registers / the history advancing captured a new graph"
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1]) and torch.equal(eager[2], graph[2])
    for a, b in zip(eager[3], graph[3]):
        assert torch.equal(a, b)
    plain = _run(gen, stream_inputs, False)
    assert torch.equal(plain[2][:5], eager[2][:5]) and float(eager[2][5][0]) == OFFSETS[0] and not torch.equal(plain[2][5:, 0], eager[2][5:, 0]), "reset([0]) left no trace"
    assert torch.equal(plain[2][5, 1:], eager[2][5, 1:]) and not torch.equal(plain[2][6:, 1:], eager[2][6:, 1:]), "the new registers left no trace"


def test_infer_streaming_auto_pitch(tmp_path, capsys):
    """`infer_streaming.py --input-wav ... --auto-pitch --streams 2`: the written file differs from the run without the flag, and equals the
    BatchedStreamInfer(auto_pitch=True) loop over the same blocks under the same seed."""
    import infer
    import infer_streaming
    from tinyvc_amd.module.infer import BatchedStreamInfer
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchRegister, PitchTrack, attach_register, save_register
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(500, seed=2), d / "index.pt")
    save_register(d / "index.pt", PitchRegister(torch.tensor([233.0]), torch.tensor([100], dtype=torch.int32)))
    audio_io.save(str(d / "mic.wav"), synth.synth_wave(3, N_BLOCKS * 1920, seed=50)[0:1] * 0.9, 24000)
    common = ["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "index.pt"), "--input-wav", str(d / "mic.wav"), "--streams", "2",
              "-d", DEV, "-p", "0.5"]
    live = ["--auto-pitch", "--auto-pitch-warmup", "0.1", "--auto-pitch-window", "10"]
    torch.manual_seed(3)
    assert infer_streaming.main(common + live + ["--output-wav", str(d / "auto.wav")]) == 0
    text = capsys.readouterr().out
    assert "stream 0: register" in text and "stream 1: register" in text and "p50" in text
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--output-wav", str(d / "plain.wav")]) == 0
    assert open(d / "auto.wav", "rb").read() != open(d / "plain.wav", "rb").read(), "--auto-pitch changed nothing"
    # the same blocks through the classes
    torch.manual_seed(3)
    dev = torch.device(DEV)
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), dev)
    tgt = attach_register(torch.load(d / "index.pt").to(dev), d / "index.pt")
    track = PitchTrack(2, 4, lag_frames=8, window_frames=500, min_voiced=5, slew=6.0 * 1920 / 24000, device=dev)
    st = BatchedStreamInfer(gen, n_streams=2, pitch_shift=0.5, block_size=1920, device=dev, extra_size=3840, auto_pitch=True, pitch_track=track)
    st.target = tgt
    st.init_buffer()
    eng = gen.engine(dev)
    outs = []
    for blk in infer_streaming.int16_blocks_from_wav(str(d / "mic.wav"), 24000, 1920, eng):
        x = eng.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(blk)).to(dev), 0)
        outs.append(eng.f32_to_pcm16(st.audio_callback(x.expand(2, -1)), 0).cpu().numpy()[0])
    assert len(outs) == N_BLOCKS and int(track.count[0]) > 5 and abs(float(st.last_pitch_shift[0]) - 0.5) > 0.2
    audio_io.save(str(d / "want.wav"), torch.from_numpy(np.concatenate(outs).astype(np.float32) / 32768)[None], 24000)
    assert open(d / "auto.wav", "rb").read() == open(d / "want.wav", "rb").read()
