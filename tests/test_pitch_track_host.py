"""The per-stream pitch tracker (feature_retrieval.PitchTrack, tvc_pitch_track_f32, tvc_convert_track_f32, Generator.convert(track=...),
BatchedStreamInfer(auto_pitch=...), infer_streaming.py --auto-pitch) without a GPU: arguments are refused on the host before anything is
allocated or any engine is involved, the entry script parses its flags and refuses their conflicts, the symbols are declared and exported.

`TrackModel` below is the CPU model of the kernel's steps 1 - 6 (include/tinyvc_hip.h): a Python list per stream, `hist = (hist + voiced)[-W:]`,
torch.median, and a ring filled one value at a time.  It is the truth of tests/test_gpu_pitch_track.py, which imports it; here it is held
against cases written out by hand."""
import math

import numpy as np
import pytest
import torch

from tinyvc_amd import _lib

NEW = ["tvc_pitch_track_f32", "tvc_convert_track_f32"]
F32 = np.float32


class TrackModel:
    """S streams, a window of W voiced frames.  step(new, target, offsets) takes the block's new frames (S rows of fp32 values: zeros,
    negatives and NaN are unvoiced) and returns (medians, shifts) as fp32 arrays; ring [S, W], count [S] and auto [S] are the state the
    device must hold afterwards.  fp32 arithmetic where the kernel's is fp32, the shift's logarithm in fp64 rounded once."""

    def __init__(self, S, W, min_voiced=1, slew=math.inf):
        self.S, self.W, self.min_voiced, self.slew = S, W, min_voiced, F32(slew)
        self.hist = [[] for _ in range(S)]
        self.ring = np.zeros((S, W), dtype=F32)
        self.count = np.zeros(S, dtype=np.int64)
        self.auto = np.zeros(S, dtype=F32)
        self.wanted = np.zeros(S, dtype=F32)

    def reset(self, streams=None):
        for s in (range(self.S) if streams is None else streams):
            self.hist[s] = []
            self.ring[s] = 0
            self.count[s] = 0
            self.auto[s] = 0

    def step(self, new, target, offsets):
        med, shift = np.zeros(self.S, dtype=F32), np.zeros(self.S, dtype=F32)
        for s in range(self.S):
            row = np.asarray(new[s], dtype=F32).reshape(-1)
            with np.errstate(invalid="ignore"):
                voiced = row[row > 0].tolist()                              # NaN > 0 is False; fp32 values as Python floats (exact)
            for x in voiced:                                                # one at a time: the definition of the ring
                self.ring[s, self.count[s] % self.W] = x
                self.count[s] += 1
            self.hist[s] = (self.hist[s] + voiced)[-self.W:]
            fill = min(int(self.count[s]), self.W)
            assert fill == len(self.hist[s])
            med[s] = F32(torch.median(torch.tensor(self.hist[s], dtype=torch.float32)).item()) if fill else F32(0)
            tg = F32(target[s])
            wanted = F32(12.0 * np.log2(np.float64(tg) / np.float64(med[s]))) if fill >= self.min_voiced and tg > 0 else F32(0)
            a = self.auto[s]
            d = F32(wanted - a)
            a = F32(a + np.copysign(self.slew, d)) if abs(d) > self.slew else wanted
            self.auto[s], self.wanted[s] = a, wanted
            shift[s] = F32(F32(offsets[s]) + a)
        return med, shift


# ---- the model against cases written out by hand -----------------------------------------------------------------------------------------
def test_model_eviction_order():
    m = TrackModel(1, 3)
    med, _ = m.step([[100.0, 0.0, 200.0, -5.0, 300.0]], [0.0], [0.0])
    assert m.ring.tolist() == [[100.0, 200.0, 300.0]] and m.count.tolist() == [3] and med.tolist() == [200.0]
    med, _ = m.step([[400.0, float("nan"), 500.0]], [0.0], [0.0])
    assert m.ring.tolist() == [[400.0, 500.0, 300.0]] and m.count.tolist() == [5], "the oldest two (100, 200) leave first"
    assert m.hist[0] == [300.0, 400.0, 500.0] and med.tolist() == [400.0]
    # more voiced frames in one block than the ring holds: the last W survive, in the slots a one-by-one append leaves them in
    m = TrackModel(1, 2)
    med, _ = m.step([[1.0, 2.0, 3.0, 4.0, 5.0]], [0.0], [0.0])
    assert m.ring.tolist() == [[5.0, 4.0]] and m.count.tolist() == [5] and med.tolist() == [4.0]      # lower median of {4, 5}
    m = TrackModel(1, 4)
    med, _ = m.step([[30.0, 10.0]], [0.0], [0.0])
    assert med.tolist() == [10.0] and m.ring.tolist() == [[30.0, 10.0, 0.0, 0.0]], "the LOWER median of an even fill; unwritten slots stay 0"


def test_model_landing_and_warmup():
    m = TrackModel(2, 8, min_voiced=3)
    _, sh = m.step([[110.0, 110.0], [110.0, 110.0]], [220.0, 220.0], [0.5, -1.0])
    assert m.auto.tolist() == [0.0, 0.0] and sh.tolist() == [0.5, -1.0], "before min_voiced values are in the ring the shift is the offset"
    _, sh = m.step([[110.0], [0.0]], [220.0, 220.0], [0.5, -1.0])
    assert m.auto.tolist() == [12.0, 0.0] and sh.tolist() == [12.5, -1.0], "slew = inf lands at once; stream 1 is still warming up"
    _, sh = m.step([[0.0], [110.0]], [0.0, float("nan")], [0.5, -1.0])
    assert m.auto.tolist() == [0.0, 0.0] and sh.tolist() == [0.5, -1.0], "no target register: no automatic shift"


def test_model_ramping():
    up, down, still = TrackModel(1, 4, slew=0.25), TrackModel(1, 4, slew=0.25), TrackModel(1, 4, slew=0.0)
    for k in range(1, 48):
        up.step([[110.0]], [220.0], [0.0])
        down.step([[220.0]], [110.0], [0.0])
        still.step([[110.0]], [220.0], [0.0])
        assert up.auto[0] == 0.25 * k and down.auto[0] == -0.25 * k and still.auto[0] == 0.0
    for _ in range(3):      # step 48 lands on 12 exactly and stays
        _, sh = up.step([[110.0]], [220.0], [1.0])
        down.step([[220.0]], [110.0], [0.0])
        assert up.auto[0] == 12.0 and down.auto[0] == -12.0 and sh[0] == 13.0
    # a target that is no multiple of the slew away: the last step is shorter, and lands on `wanted` itself
    m = TrackModel(1, 4, slew=0.25)
    want = F32(12.0 * np.log2(np.float64(F32(150.0)) / np.float64(F32(110.0))))      # 5.369...
    for k in range(1, 22):
        m.step([[110.0]], [150.0], [0.0])
        assert m.auto[0] == 0.25 * k
    m.step([[110.0]], [150.0], [0.0])
    assert m.auto[0] == want and m.wanted[0] == want


# ---- PitchTrack: every argument is checked before anything is allocated ---------------------------------------------------------------------
@pytest.mark.parametrize("kw, match", [
    (dict(window_frames=0), "window_frames"), (dict(window_frames=8193), "window_frames"),
    (dict(new_frames=-1), "new_frames"), (dict(new_frames=257), "new_frames"),
    (dict(min_voiced=0), "min_voiced"), (dict(slew=-0.5), "slew"), (dict(slew=float("nan")), "slew"),
    (dict(n_streams=0), "n_streams"), (dict(lag_frames=-1), "lag_frames"), (dict(window_frames=10.5), "window_frames"),
])
@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_pitch_track_refuses_before_allocating(kw, match, device, monkeypatch):
    """ValueError on the host, whatever the device: `cuda` on a box without a GPU must not get as far as a device error.  torch.zeros is
    replaced by a function that fails the test: nothing may be allocated."""
    from tinyvc_amd.module.tinyvc import feature_retrieval as fr
    monkeypatch.setattr(fr.torch, "zeros", lambda *a, **k: pytest.fail("allocated before the arguments were checked"))
    args = dict(n_streams=2, new_frames=4)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        fr.PitchTrack(device=device, **args)


def test_pitch_track_state_and_reset():
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="GPU"):
            PitchTrack(2, 4)      # the default device is the GPU: a ValueError, not a device error
    tr = PitchTrack(3, 4, lag_frames=8, window_frames=16, min_voiced=10, slew=0.25, device="cpu")
    assert tr.ring.shape == (3, 16) and tr.ring.dtype == torch.float32 and tr.count.dtype == torch.int64 and tr.auto.shape == (3,)
    assert not tr.ring.any() and not tr.count.any() and not tr.auto.any()
    assert tr.columns(28) == (16, 4) and tr.params() == (4, 8, 16, 10, 0.25)
    with pytest.raises(ValueError, match="do not fit"):
        tr.columns(11)
    assert PitchTrack(1, 0, window_frames=1, device="cpu").slew == math.inf and PitchTrack(1, 256, window_frames=8192, device="cpu").ring.shape == (1, 8192)
    ptrs = (tr.ring.data_ptr(), tr.count.data_ptr(), tr.auto.data_ptr())
    tr.ring.fill_(100.0), tr.count.fill_(7), tr.auto.fill_(1.5)
    tr.reset([1])
    assert tr.ring[1].tolist() == [0.0] * 16 and tr.count.tolist() == [7, 0, 7] and tr.auto.tolist() == [1.5, 0.0, 1.5] and bool((tr.ring[0] == 100.0).all())
    tr.reset()
    assert not tr.ring.any() and not tr.count.any() and not tr.auto.any()
    assert ptrs == (tr.ring.data_ptr(), tr.count.data_ptr(), tr.auto.data_ptr()), "reset must work in place: a captured graph holds these addresses"


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_symbols_are_declared_and_exported(lib):
    from test_cabi import header_functions
    decl = header_functions()
    for name in NEW:
        assert name in decl, f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl[name]), name
        assert hasattr(lib, name), f"{name} is not exported"
    # argument checks come before any device work: no context, no call
    assert lib.tvc_pitch_track_f32(None, None, None, 1, 28, 16, 4, None, 0.0, None, 1500, 25, 0.0, None, None, None, None, None, None, None) == -1
    assert lib.tvc_convert_track_f32(None, None, None, None, None, 1, None, None, 16, 4, 1500, 25, 0.0, None, None, None, 0.0, None, None, None, 0, None,
                                     1, 13440, None, 0) == -1
    from tinyvc_amd import spec
    from tinyvc_amd.engine import _CONVERT, Engine
    assert callable(Engine.pitch_track) and _CONVERT["track", False] == ("tvc_workspace_bytes_auto", "tvc_convert_track_f32") and ("track", True) not in _CONVERT
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinyvc_hip.h")).read()
    assert re.search(r"#define\s+TVC_PITCH_TRACK_MAX_WINDOW\s+8192\b", header) and spec.PITCH_TRACK_MAX_WINDOW == 8192


# ---- Generator.convert and the stream classes: refusals before any engine work -------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_gen():
    """a Generator that never left the CPU: whatever reaches its engine raises TinyVCError (a RuntimeError), never ValueError"""
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_convert_refusals_come_before_device_work(cpu_gen):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    wf = torch.zeros(2, 28 * 480)
    plain = torch.zeros(1, 768, 8)
    track = PitchTrack(2, 4, lag_frames=8, device="cpu")
    with pytest.raises(ValueError, match="track needs auto_pitch"):
        cpu_gen.convert(wf, plain, 0.0, track=track)
    with pytest.raises(ValueError, match="track with lengths"):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch=200.0, lengths=[9600, 13440], track=track)
    with pytest.raises(ValueError, match="a tracker of 3 streams for a batch of 2"):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch=200.0, track=PitchTrack(3, 4, device="cpu"))
    with pytest.raises(ValueError, match="do not fit T = 11"):
        cpu_gen.convert(wf[:, :11 * 480 - 7], plain, 0.0, auto_pitch=200.0, track=track)      # padded to 11 frames; 8 + 4 are needed
    # a well-formed call gets as far as the device - and there is none
    with pytest.raises(_lib.TinyVCError):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch=200.0, track=track, return_shift=True)


def test_stream_constructors(cpu_gen):
    import inspect
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    for cls in (BatchedStreamInfer, StreamInfer):
        assert list(inspect.signature(cls.__init__).parameters)[-2:] == ["auto_pitch", "pitch_track"], "the new keywords go last"
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="480"):
        BatchedStreamInfer(cpu_gen, 2, device=dev, block_size=1000, auto_pitch=200.0)
    with pytest.raises(ValueError, match="pitch_track needs auto_pitch"):
        BatchedStreamInfer(cpu_gen, 2, device=dev, pitch_track=PitchTrack(2, 4, device="cpu"))
    st = BatchedStreamInfer(cpu_gen, 2, device=dev, block_size=1000)      # without auto_pitch nothing changes
    assert st.auto_pitch is None and st.pitch_track is None and st.last_pitch_shift is None


# ---- infer_streaming.py: the flags and their conflicts ------------------------------------------------------------------------------------------
def test_entry_script_flags_and_conflicts():
    import infer_streaming
    parse = infer_streaming.build_parser().parse_args
    a = parse([])
    assert a.auto_pitch is False and a.auto_pitch_window == 30.0 and a.auto_pitch_warmup == 0.5 and a.auto_pitch_slew == 6.0
    assert infer_streaming.check_auto_pitch(a) is None
    a = parse(["--auto-pitch", "-p", "2.5"])
    assert a.auto_pitch is True and a.pitch_shift == 2.5 and a.auto_pitch_from is None
    kw = infer_streaming.check_auto_pitch(a)
    assert kw == dict(new_frames=4, window_frames=1500, min_voiced=25, slew=6.0 * 1920 / 24000)      # semitones per 80 ms block
    kw = infer_streaming.check_auto_pitch(parse(["--auto-pitch", "--auto-pitch-slew", "0", "--auto-pitch-window", "2", "--auto-pitch-warmup", "0", "-c", "960"]))
    assert kw == dict(new_frames=2, window_frames=100, min_voiced=1, slew=math.inf)
    assert parse(["--auto-pitch-from", "calib.wav"]).auto_pitch is False
    for argv in (["--auto-pitch", "--auto-pitch-from", "calib.wav"], ["--auto-pitch", "--blend", "a.pt=0.5", "b.pt=0.5"], ["--auto-pitch", "-c", "1000"],
                 ["--auto-pitch", "--auto-pitch-window", "200"], ["--auto-pitch", "--auto-pitch-slew", "-1"]):
        with pytest.raises(SystemExit) as e:
            infer_streaming.check_auto_pitch(parse(argv))
        assert "--auto-pitch" in str(e.value.code), argv
    text = infer_streaming.build_parser().format_help()
    assert "guesses" in text, "the help must say that nobody has listened to the defaults"
