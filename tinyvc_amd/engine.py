"""Thin host-side wrapper around one `tvc_ctx` (one per device and weight set).

PyTorch is used here for device memory (tensors in, tensors out), the current HIP stream and the
scratch workspace; every computation is a call into libtinyvc_hip.so.
"""
import collections
import ctypes
import math
import numbers
import threading
import types
import weakref

import torch

from . import _lib, spec
from .stream_state import CARRY_STATE, DENOISE_STATE, GATE_STATE, LIMITER_STATE, LOUDNESS_STATE, SNAP_STATE, TRACK_STATE, Field, checked

_F32 = torch.float32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _floats(xs):
    return (ctypes.c_float * len(xs))(*xs) if xs is not None else None


def _check_dev(t, name, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise _lib.TinyVCError(
            f"{name} is on {t.device}: tinyvc_amd runs on an AMD GPU only (no CPU fallback). "
            "Move the model and inputs to 'cuda'.")
    if device is not None and t.device != device:
        raise _lib.TinyVCError(f"{name} is on {t.device}, engine is on {device}")


def _prep(t, name, device):
    _check_dev(t, name, device)
    if t.dtype != _F32:
        t = t.float()
    return t.contiguous()


def integer(x, what, name):
    """x as the int a C int argument takes; ValueError for a bool, anything that is no integer (240.9 is not 240) or one beyond 32 bits"""
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or abs(x) >= 2 ** 31:
        raise ValueError(f"{what}: {name} must be an integer, got {x!r}")
    return int(x)


def pitch_shifts(pitch_shift, B):
    """convert's pitch_shift, parsed on the host (no device work): a float / 0-d tensor -> (pitch_shift, None); a sequence / 1-D tensor of one
    shift per row -> (0.0, [B floats]).  ValueError for any other form or length."""
    if isinstance(pitch_shift, torch.Tensor):
        if pitch_shift.dim() == 0:
            return float(pitch_shift), None
        if pitch_shift.dim() != 1:
            raise ValueError("pitch_shift: a float or a 1-D sequence of one shift per row")
        pitch_shift = pitch_shift.detach().cpu().tolist()
    if not hasattr(pitch_shift, "__len__"):
        return float(pitch_shift), None
    sh = [float(x) for x in pitch_shift]
    if len(sh) != B:
        raise ValueError(f"pitch_shift: {len(sh)} shifts for a batch of {B}")
    return 0.0, sh


# the C names of a conversion / a match: (how the index is given, ragged) -> (tvc_workspace_bytes* query, entry).  Nothing else decides them.
_CONVERT = {
    ("shared", False): ("tvc_workspace_bytes", "tvc_convert_f32"),
    ("shared", True): ("tvc_workspace_bytes_ragged", "tvc_convert_ragged_f32"),
    ("table", False): ("tvc_workspace_bytes_multi", "tvc_convert_multi_f32"),
    ("table", True): ("tvc_workspace_bytes_ragged_multi", "tvc_convert_ragged_multi_f32"),
    ("blend", False): ("tvc_workspace_bytes_blend", "tvc_convert_blend_f32"),
    ("blend", True): ("tvc_workspace_bytes_ragged_blend", "tvc_convert_ragged_blend_f32"),
    ("auto", False): ("tvc_workspace_bytes_auto", "tvc_convert_auto_f32"),
    ("auto", True): ("tvc_workspace_bytes_ragged_auto", "tvc_convert_ragged_auto_f32"),
    ("track", False): ("tvc_workspace_bytes_auto", "tvc_convert_track_f32"),      # streams advance in lock step: no ragged form
    ("alpha", False): ("tvc_workspace_bytes_alpha", "tvc_convert_alpha_f32"),      # any table / blend call, with or without auto pitch and a tracker, + alpha
    ("alpha", True): ("tvc_workspace_bytes_ragged_alpha", "tvc_convert_ragged_alpha_f32"),
}
_MATCH = {
    "shared": ("tvc_workspace_bytes", "tvc_knn_match_f32"),
    "table": ("tvc_workspace_bytes_multi", "tvc_knn_match_multi_f32"),
    "blend": ("tvc_workspace_bytes_blend", "tvc_knn_match_blend_f32"),
    "alpha": ("tvc_workspace_bytes_alpha", "tvc_knn_match_alpha_f32"),
}
# form "protect": the alpha rows' calls with `protect` behind alpha (and f0 behind the stage call's src) - (ragged,) for a conversion, "match"
_PROTECT = {
    False: ("tvc_workspace_bytes_protect", "tvc_convert_protect_f32"),
    True: ("tvc_workspace_bytes_ragged_protect", "tvc_convert_ragged_protect_f32"),
    "match": ("tvc_workspace_bytes_protect", "tvc_knn_match_protect_f32"),
}


# form "path": the protect rows' conversions with the pitch path's settings behind protect - (ragged,)
_PATH = {
    False: ("tvc_workspace_bytes_path", "tvc_convert_path_f32"),
    True: ("tvc_workspace_bytes_ragged_path", "tvc_convert_ragged_path_f32"),
    "carry": ("tvc_workspace_bytes_path", "tvc_convert_carry_f32"),      # the path's state from block to block: streams advance in lock step, no ragged form
}


# form "tuned": the carry call / the ragged path call with the pitch correction in front of the decoder; everything behind the index is
# optional there, the carry included - (ragged,)
_TUNED = {
    False: ("tvc_workspace_bytes_path", "tvc_tuned_convert_f32"),
    True: ("tvc_workspace_bytes_ragged_path", "tvc_tuned_convert_ragged_f32"),
}


# form "weighted": the tuned rows' conversions / the protect match with neighbours and width behind protect; everything behind the index is
# optional, as there - (ragged,) for a conversion, "match".  No query of its own: the weights take no workspace.
_WEIGHTED = {
    False: ("tvc_workspace_bytes_path", "tvc_weighted_convert_f32"),
    True: ("tvc_workspace_bytes_ragged_path", "tvc_weighted_convert_ragged_f32"),
    "match": ("tvc_workspace_bytes_protect", "tvc_knn_match_weighted_f32"),
}


# form "joined": the weighted rows' calls with the continuity weight `join` behind width - the match along a path.  The path takes workspace:
# queries of its own.
_JOINED = {
    False: ("tvc_workspace_bytes_joined", "tvc_joined_convert_f32"),
    True: ("tvc_workspace_bytes_ragged_joined", "tvc_joined_convert_ragged_f32"),
    "match": ("tvc_workspace_bytes_match_joined", "tvc_knn_match_joined_f32"),
}


def _names(form, ragged=None):
    """(workspace query, entry) of a conversion (`ragged` a bool) or a match (None) from the tables above"""
    if form == "joined":
        return _JOINED["match" if ragged is None else ragged]
    if form == "weighted":
        return _WEIGHTED["match" if ragged is None else ragged]
    if form == "tuned":
        return _TUNED[ragged]
    if form == "path":
        return _PATH[ragged]
    if form == "protect":
        return _PROTECT["match" if ragged is None else ragged]
    return _MATCH[form] if ragged is None else _CONVERT[form, ragged]


# a tracker's and a carry's share of a call, and every optional parameter of a conversion at its "off" value: the C parameters' names
_TrackArgs = collections.namedtuple("_TrackArgs", "start n W min_voiced slew ring count auto_shift")
_CarryArgs = collections.namedtuple("_CarryArgs", "carry_frame carry")
_SnapArgs = collections.namedtuple("_SnapArgs", "snap notes strength snap_carry_frame snap_note snap_ratio")
_FEATURES_OFF = dict(lens=None, M=0, weights=None, alpha=None, protect=None, neighbours=None, width=None, join=None, path=None, target_f0=None, shift_out=None,
                     **_CarryArgs(0, None)._asdict(), **_SnapArgs(None, None, None, 0, None, None)._asdict(), **_TrackArgs(0, 0, 0, 0, 0.0, None, None, None)._asdict())


_RESAMPLE_STATE =(Field("state", _F32, "hist", 0.0),)      # what stream_resample takes of a door: one side's history
STREAM_RESAMPLE_LDS_FLOATS = 16384      # TVC_STREAM_RESAMPLE_LDS_FLOATS of tinyvc_hip.h: a stream's history + block, staged in 64 KiB of LDS


def stream_resample_geometry(in_freq, out_freq, n_in, lib=None):
    """tvc_stream_resample_geometry (no context, no device) -> (n_out, hist, delay) for blocks of n_in samples at in_freq, resampled to out_freq.
    ValueError, with the reason, for what the library refuses."""
    in_freq, out_freq, n_in = int(in_freq), int(out_freq), int(n_in)
    lib = lib if lib is not None else _lib.load_library()
    n_out, hist, delay = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    if lib.tvc_stream_resample_geometry(in_freq, out_freq, n_in, ctypes.byref(n_out), ctypes.byref(hist), ctypes.byref(delay)) != 0:
        if in_freq <= 0 or out_freq <= 0 or n_in <= 0:
            raise ValueError(f"stream resample: rates and block length must be positive, got {in_freq} -> {out_freq} Hz, n_in = {n_in}")
        orig = in_freq // math.gcd(in_freq, out_freq)
        if n_in % orig:
            raise ValueError(f"stream resample: {in_freq} -> {out_freq} Hz takes blocks of whole {orig}-sample groups; n_in = {n_in} is not one")
        raise ValueError(f"stream resample: a block of {n_in} samples at {in_freq} -> {out_freq} Hz and its history do not fit the kernel's LDS budget of "
                         f"{STREAM_RESAMPLE_LDS_FLOATS} floats (64 KiB per stream)")
    return n_out.value, hist.value, delay.value


SOLA_CROSS, SOLA_SEARCH, SOLA_DELAY = 1920, 1920, 3840      # the reference's SOLA geometry (stream.py:48-50): the defaults, and the caps of the first two


def sola_geometry(block, cross=SOLA_CROSS, search=SOLA_SEARCH, delay=SOLA_DELAY, lib=None):
    """tvc_sola_geometry (no context, no device) -> (min_ly, latency_min, latency_max) of a streaming tail with `block`-sample blocks: the
    shortest converted buffer it takes, and the range of cross + search + delay - shift, in 24 kHz samples.  ValueError, with the library's
    reason, for a geometry the kernels do not take."""
    block, cross, search, delay = (integer(x, "sola geometry", name) for x, name in ((block, "block"), (cross, "cross"), (search, "search"), (delay, "delay")))
    lib = lib if lib is not None else _lib.load_library()
    min_ly, lo, hi = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    if lib.tvc_sola_geometry(block, cross, search, delay, ctypes.byref(min_ly), ctypes.byref(lo), ctypes.byref(hi)) != 0:
        raise ValueError(f"sola geometry: {lib.tvc_sola_geometry_message(block, cross, search, delay).decode()}")
    return min_ly.value, lo.value, hi.value


def stream_gate_geometry(block, sub, look=0, hold=0, attack=1, release=1, lib=None):
    """tvc_stream_gate_geometry (no context, no device) -> (nsub, look_samples) of a noise gate over `block`-sample blocks in sub-frames of
    `sub` samples; look, hold, attack and release count sub-frames.  ValueError, with the library's reason, for what the kernel does not take."""
    vals = tuple(integer(x, "stream gate geometry", name)
                 for x, name in zip((block, sub, look, hold, attack, release), ("block", "sub", "look", "hold", "attack", "release")))
    lib = lib if lib is not None else _lib.load_library()
    nsub, look_samples = ctypes.c_int(), ctypes.c_int()
    if lib.tvc_stream_gate_geometry(*vals, ctypes.byref(nsub), ctypes.byref(look_samples)) != 0:
        raise ValueError(f"stream gate geometry: {lib.tvc_stream_gate_geometry_message(*vals).decode()}")
    return nsub.value, look_samples.value


def stream_denoise_geometry(block, hop=160, lib=None):
    """tvc_stream_denoise_geometry (no context, no device) -> (frames, delay) of a spectral suppressor over `block`-sample blocks at a hop of
    `hop` samples: frames per block and the samples of delay it adds (640 - hop).  ValueError, with the library's reason, for what the
    kernel does not take."""
    block, hop = integer(block, "stream denoise geometry", "block"), integer(hop, "stream denoise geometry", "hop")
    lib = lib if lib is not None else _lib.load_library()
    frames, delay = ctypes.c_int(), ctypes.c_int()
    if lib.tvc_stream_denoise_geometry(block, hop, ctypes.byref(frames), ctypes.byref(delay)) != 0:
        raise ValueError(f"stream denoise geometry: {lib.tvc_stream_denoise_geometry_message(block, hop).decode()}")
    return frames.value, delay.value


def loudness_geometry(length, sub=240, smooth=2, stream_block=False, lib=None):
    """tvc_loudness_geometry (no context, no device) -> (nsub, window, tile) of a loudness match over `length` samples in sub-frames of `sub`
    samples with `smooth` sub-frames each side: sub-frames, window = 2 * smooth + 1, and the sub-frames a workgroup of the offline form owns.
    stream_block: `length` is a stream's block (tvc_stream_loudness_geometry: at most 4096 sub-frames; tile is None).  ValueError, with the
    library's reason, for what the kernels do not take."""
    if isinstance(length, bool) or not isinstance(length, numbers.Integral) or abs(length) >= (2 ** 31 if stream_block else 2 ** 63):
        raise ValueError(f"loudness geometry: length must be an integer, got {length!r}")
    vals = (int(length), integer(sub, "loudness geometry", "sub"), integer(smooth, "loudness geometry", "smooth"))
    lib = lib if lib is not None else _lib.load_library()
    nsub, window, tile = (ctypes.c_int if stream_block else ctypes.c_int64)(), ctypes.c_int(), ctypes.c_int()
    if stream_block:
        if lib.tvc_stream_loudness_geometry(*vals, ctypes.byref(nsub), ctypes.byref(window)) != 0:
            raise ValueError(f"loudness geometry: {lib.tvc_stream_loudness_geometry_message(*vals).decode()}")
        return nsub.value, window.value, None
    if lib.tvc_loudness_geometry(*vals, ctypes.byref(nsub), ctypes.byref(window), ctypes.byref(tile)) != 0:
        raise ValueError(f"loudness geometry: {lib.tvc_loudness_geometry_message(*vals).decode()}")
    return nsub.value, window.value, tile.value


def loudness_levels(floor_db=-60.0, boost_db=12.0, cut_db=40.0, what="loudness"):
    """the three dB settings of a loudness match as the fp32 values the library takes; ValueError for what it refuses: a floor that is not
    finite, a boost or cut that is negative or not finite (they are the most the gain may raise or lower a sub-frame by)"""
    vals = []
    for x, name, least in ((floor_db, "floor_db", None), (boost_db, "boost_db", 0.0), (cut_db, "cut_db", 0.0)):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or (least is not None and x < least):
            raise ValueError(f"{what}: {name} must be a finite number of dB" + ("" if least is None else " >= 0") + f", got {x!r}")
        v = ctypes.c_float(x).value
        if not math.isfinite(v) or abs(v) > 600.0:      # 10^(+-30) as an fp32 gain, 10^(+-60) as a power: far inside what the library takes
            raise ValueError(f"{what}: {name} = {x!r} dB is outside -600 .. 600")
        vals.append(v)
    return tuple(vals)


def loudness_in_place(rows, device):
    """whether a loudness match of `rows` rows should run in place: an in-place call is one workgroup per row (a tile's halo lies in tiles
    another workgroup would be scaling), so it pays once the rows alone fill the device's compute units; below that a call into a tensor of
    its own, rows x tiles workgroups, is faster (64 x 4 s: 35 us against 154 us; one five-minute row: profiles/loudness_probe.json)"""
    return rows >= torch.cuda.get_device_properties(device).multi_processor_count


def limiter_geometry(length, sub=24, release=100, stream_block=False, lib=None):
    """tvc_limiter_geometry (no context, no device) -> (nsub, delay, tile) of a peak limiter over `length` samples in sub-frames of `sub`
    samples with a release of `release` sub-frames: sub-frames, the delay of the stream form in samples (= sub), and the sub-frames a
    workgroup of the offline form owns.  stream_block: `length` is a stream's block (tvc_stream_limiter_geometry; the third value is then
    the chunk of sub-frames the stream kernel walks a block in).  ValueError, with the library's reason, for what the kernels do not take."""
    if isinstance(length, bool) or not isinstance(length, numbers.Integral) or abs(length) >= (2 ** 31 if stream_block else 2 ** 63):
        raise ValueError(f"limiter geometry: length must be an integer, got {length!r}")
    vals = (int(length), integer(sub, "limiter geometry", "sub"), integer(release, "limiter geometry", "release"))
    lib = lib if lib is not None else _lib.load_library()
    nsub, delay, tile = (ctypes.c_int if stream_block else ctypes.c_int64)(), ctypes.c_int(), ctypes.c_int()
    name = "tvc_stream_limiter_geometry" if stream_block else "tvc_limiter_geometry"
    if getattr(lib, name)(*vals, ctypes.byref(nsub), ctypes.byref(delay), ctypes.byref(tile)) != 0:
        raise ValueError(f"limiter geometry: {getattr(lib, name + '_message')(*vals).decode()}")
    return nsub.value, delay.value, tile.value


def limiter_drive(drive_db=0.0, what="limiter"):
    """a limiter's drive_db as the fp32 value the library takes; ValueError for a drive that is not a finite number of dB within +-600 (the
    library itself refuses only a factor 10^(drive_db / 20) that is not a positive finite fp32 number)"""
    if isinstance(drive_db, bool) or not isinstance(drive_db, (int, float)) or not math.isfinite(drive_db):
        raise ValueError(f"{what}: drive_db must be a finite number of dB, got {drive_db!r}")
    v = ctypes.c_float(drive_db).value
    if not math.isfinite(v) or abs(v) > 600.0:      # 10^(+-30) as an fp32 factor: far inside what the library takes
        raise ValueError(f"{what}: drive_db = {drive_db!r} dB is outside -600 .. 600")
    return v


def pitch_class_table():
    """PitchEstimator.id2freq over ids 0..511 (reference encoder.py:48-54), on the host."""
    ids = torch.arange(spec.PITCH_CLASSES).to(torch.float)
    x = spec.PITCH_FMIN * (2 ** (ids / spec.PITCH_CPO))
    x[x <= spec.PITCH_FMIN] = 0
    return x.contiguous()


def _forget_blob(engine_ref, ptr):
    eng = engine_ref()
    if eng is not None and getattr(eng, "ctx", None):
        eng.lib.tvc_knn_forget(eng.ctx, ctypes.c_void_p(ptr))


class Engine:
    """Owns a tvc_ctx on `device`, its weights and a grow-only scratch workspace."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.TinyVCError(f"tinyvc_amd needs a GPU device, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.lib = _lib.load_library()
        h = ctypes.c_void_p()
        rc = self.lib.tvc_ctx_create(device.index, ctypes.byref(h))
        if rc != 0 or not h:
            raise _lib.TinyVCError(f"tvc_ctx_create(device={device.index}) failed with {rc}")
        self.ctx = h
        self._ws = None
        self._seed = 0x1234ABCD
        self.weights_key = None

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.tvc_ctx_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _ok(self, rc, what):
        if rc != 0:
            msg = self.lib.tvc_last_error(self.ctx)
            raise _lib.TinyVCError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _grow_ws(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _query_ws(self, query, *args, **named):
        """Ask the tvc_workspace_bytes* function `query` what the call described by `args` (in its order), or by `named` (under its
        parameters' names: _lib.arguments), needs and grow the workspace to it -> (pointer, size): the last two arguments of the entry
        that query belongs to."""
        need = ctypes.c_size_t()
        args = _lib.arguments(query, dict(named, ctx=self.ctx, out_bytes=ctypes.byref(need))) if named else (self.ctx, *args, ctypes.byref(need))
        self._ok(getattr(self.lib, query)(*args), query)
        ws = self._grow_ws(need.value)
        return _ptr(ws), ctypes.c_size_t(ws.numel())

    def workspace(self, B, L, N):
        self._query_ws("tvc_workspace_bytes", int(B), int(L), int(max(N, 4)))
        return self._ws

    def _wsargs(self, B, L, N=4):
        ws = self.workspace(B, L, N)
        return _ptr(ws), ctypes.c_size_t(ws.numel())

    def set_ragged_batch_frames(self, max_frames):
        """Frames per in-kernel batch of this engine's ragged calls (0 = the default, 80 000); results do not depend on it."""
        self._ok(self.lib.tvc_ctx_set_ragged_batch_frames(self.ctx, int(max_frames)), "tvc_ctx_set_ragged_batch_frames")

    def set_index_assign_chunk(self, max_queries):
        """Points per search call of this engine's index_assign / index_compact (0 = the default, 32 768); results do not depend on it."""
        self._ok(self.lib.tvc_ctx_set_index_assign_chunk(self.ctx, int(max_queries)), "tvc_ctx_set_index_assign_chunk")

    def next_seed(self):
        self._seed = (self._seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self._seed

    def profile(self, on=True):
        """Bracket stages with hipEvents on the launch stream (see tvc_profile_read): True / 1 = every stage and FilterNet block,
        2 = the `filter_net` region only, False / 0 = off."""
        self._ok(self.lib.tvc_profile_enable(self.ctx, int(on)), "tvc_profile_enable")

    def profile_read(self):
        """{region: milliseconds} summed since the last read; synchronises the recorded events."""
        buf = ctypes.create_string_buffer(8192)
        self._ok(self.lib.tvc_profile_read(self.ctx, buf, len(buf)), "tvc_profile_read")
        out = {}
        for item in buf.value.decode().split(";"):
            if "=" in item:
                k, v = item.split("=")
                out[k] = float(v)
        return out

    # ------------------------------------------------------------------ weights
    def load_weights(self, tensors):
        """tensors: {state_dict key: tensor} for an encoder, a decoder or both."""
        keep = []
        for k, v in tensors.items():
            t = v.detach().to("cpu", _F32).contiguous()
            keep.append(t)
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            self._ok(self.lib.tvc_load_tensor(self.ctx, k.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()), f"tvc_load_tensor({k})")
        tab = pitch_class_table()
        self._ok(self.lib.tvc_set_pitch_table(self.ctx, ctypes.c_void_p(tab.data_ptr()), tab.numel()), "tvc_set_pitch_table")
        self._ok(self.lib.tvc_finalize_weights(self.ctx), "tvc_finalize_weights")

    # ------------------------------------------------------------------ stages
    def stft_mag(self, wav):
        wav = _prep(wav, "wave", self.device)
        B, L = wav.shape
        if L % spec.HOP:
            raise ValueError("waveform length must be a multiple of 480 (autopad_waveform)")
        out = torch.empty(B, spec.FFT_BIN, L // spec.HOP, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, L)
        self._ok(self.lib.tvc_stft_mag_f32(self.ctx, self._stream(), _ptr(wav), _ptr(out), B, L, p, n), "tvc_stft_mag_f32")
        return out

    def energy(self, wav):
        wav = _prep(wav, "wave", self.device)
        B, L = wav.shape
        out = torch.empty(B, 1, L, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, max(L - L % spec.HOP, spec.HOP))
        self._ok(self.lib.tvc_energy_f32(self.ctx, self._stream(), _ptr(wav), _ptr(out), B, L, p, n), "tvc_energy_f32")
        return out

    # ------------------------------------------------------------------ front door (entry scripts)
    def resample(self, wav, orig_freq, new_freq):
        """torchaudio.functional.resample on the device: wav [..., n] -> [..., ceil(n * new / orig)]."""
        orig_freq, new_freq = int(orig_freq), int(new_freq)
        wav = _prep(wav, "wave", self.device)
        if orig_freq == new_freq:
            return wav
        shape = wav.shape
        x = wav.reshape(-1, shape[-1])
        n_out = self.lib.tvc_resample_out_len(x.shape[1], orig_freq, new_freq)
        y = torch.empty(x.shape[0], n_out, dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_resample_f32(self.ctx, self._stream(), _ptr(x), _ptr(y), x.shape[0], x.shape[1], orig_freq, new_freq), "tvc_resample_f32")
        return y.reshape(shape[:-1] + (n_out,))

    def pcm16_to_f32(self, pcm, gain_db=0.0):
        """int16 PCM -> float in [-1, 1) (x / 32768), then torchaudio.functional.gain(gain_db) (infer_streaming.py:85-89)."""
        _check_dev(pcm, "pcm", self.device)
        if pcm.dtype != torch.int16:
            raise ValueError("pcm must be int16")
        pcm = pcm.contiguous()
        y = torch.empty(pcm.shape, dtype=_F32, device=self.device)
        if pcm.numel():
            self._ok(self.lib.tvc_pcm16_to_f32(self.ctx, self._stream(), _ptr(pcm), _ptr(y), pcm.numel(), float(gain_db)), "tvc_pcm16_to_f32")
        return y

    def f32_to_pcm16(self, x, gain_db=0.0):
        """gain(gain_db) -> * 32768 -> int16 (numpy's cast: truncation toward zero) (infer_streaming.py:91-94)."""
        x = _prep(x, "wave", self.device)
        pcm = torch.empty(x.shape, dtype=torch.int16, device=self.device)
        if x.numel():
            self._ok(self.lib.tvc_f32_to_pcm16(self.ctx, self._stream(), _ptr(x), _ptr(pcm), x.numel(), float(gain_db)), "tvc_f32_to_pcm16")
        return pcm

    def stream_resample_geometry(self, in_freq, out_freq, n_in):
        """The streaming door's geometry for blocks of `n_in` samples (tvc_stream_resample_geometry: host only) -> (n_out, hist, delay)."""
        return stream_resample_geometry(in_freq, out_freq, n_in, self.lib)

    def stream_resample_prepare(self, in_freq, out_freq):
        """Build this engine's filter table for a rate pair now (its first use allocates: not inside a graph capture)."""
        self._ok(self.lib.tvc_stream_resample_prepare(self.ctx, int(in_freq), int(out_freq)), "tvc_stream_resample_prepare")

    def stream_resample(self, x, state, in_freq, out_freq, gain_db=0.0, out_pcm16=False):
        """One block of S streams through the streaming resampler: x [S, n_in] (int16 PCM or fp32) -> [S, n_out] (int16 with out_pcm16,
        else fp32); state [S, hist] fp32 is the streams' filter history, advanced in place (None at equal rates).  gain_db goes with the
        int16 side.  The blocks of a stream, concatenated, are resample(G * orig zeros ++ its input) from the start, bit for bit."""
        _check_dev(x, "x", self.device)
        in16 = x.dtype == torch.int16
        if x.dim() != 2 or not (in16 or x.dtype == _F32):
            raise ValueError("stream_resample: x is [S, n_in], int16 or fp32")
        x = x.contiguous()
        S, n_in = x.shape
        n_out, hist, _ = self.stream_resample_geometry(in_freq, out_freq, n_in)
        if hist:      # one side of a door: the field of DOOR_STATE for this rate pair
            checked(types.SimpleNamespace(state=state, hist=hist), _RESAMPLE_STATE, S, self.device, f"stream_resample ({in_freq} -> {out_freq} Hz): ")
        y = torch.empty(S, n_out, dtype=torch.int16 if out_pcm16 else _F32, device=self.device)
        self._ok(self.lib.tvc_stream_resample(self.ctx, self._stream(), _ptr(x), int(in16), _ptr(y), int(bool(out_pcm16)), _ptr(state) if hist else None,
                                              S, n_in, int(in_freq), int(out_freq), float(gain_db)), "tvc_stream_resample")
        return y

    def encoder(self, spec_t, want_logits=False):
        x = _prep(spec_t, "spec", self.device)
        B, C, T = x.shape
        if C != spec.FFT_BIN:
            raise ValueError(f"spec must have {spec.FFT_BIN} bins, got {C}")
        ssl = torch.empty(B, spec.SSL_DIM, T, dtype=_F32, device=self.device)
        f0 = torch.empty(B, 1, T, dtype=_F32, device=self.device)
        logits = torch.empty(B, spec.PITCH_CLASSES, T, dtype=_F32, device=self.device) if want_logits else None
        p, n = self._wsargs(B, T * spec.HOP)
        self._ok(self.lib.tvc_encoder_f32(self.ctx, self._stream(), _ptr(x), _ptr(ssl), _ptr(f0), _ptr(logits), B, T, p, n), "tvc_encoder_f32")
        return ssl, f0, logits

    def pitch_decode(self, logits):
        """PitchEstimator.decode: logits [B,512,T] -> f0 [B,1,T]."""
        lg = _prep(logits, "logits", self.device)
        B, C, T = lg.shape
        if C != spec.PITCH_CLASSES:
            raise ValueError(f"logits must have {spec.PITCH_CLASSES} classes")
        f0 = torch.empty(B, 1, T, dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_pitch_decode_f32(self.ctx, self._stream(), _ptr(lg), _ptr(f0), B, T), "tvc_pitch_decode_f32")
        return f0

    def knn_prepare(self, index):
        """index: [768, N] or [1, 768, N] -> (prepared blob (1-D float tensor), N).  An fp32 index gets the fp32 storage
        (bit-exact indices on gap-checked inputs); a torch.float16 index gets the fp16 storage (2 B per element: the
        1 M-vector case).  The blob is self-describing: knn_match / convert take either."""
        _check_dev(index, "index", self.device)
        half = index.dtype == torch.float16
        idx = index if half else _prep(index, "index", self.device)
        if idx.dim() == 3:
            if idx.shape[0] != 1:
                raise ValueError("knn_prepare takes one index ([1, 768, N])")
            idx = idx[0]
        if idx.shape[0] != spec.SSL_DIM:
            raise ValueError(f"index must be [768, N], got {tuple(idx.shape)}")
        N = idx.shape[1]
        if N < 4:
            raise RuntimeError("selected index k out of range")  # what torch.topk raises in the reference
        if half:
            rows = idx.t().contiguous()          # [N, 768] half, one vector per row
            blob = torch.empty(self.lib.tvc_knn_prepared_elems_f16(N), dtype=_F32, device=self.device)
            self._ok(self.lib.tvc_knn_prepare_index_f16(self.ctx, self._stream(), _ptr(rows), _ptr(blob), N), "tvc_knn_prepare_index_f16")
            return self._owned(blob), N
        blob = torch.empty(self.lib.tvc_knn_prepared_elems(N), dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_knn_prepare_index_f32(self.ctx, self._stream(), _ptr(idx.contiguous()), _ptr(blob), N), "tvc_knn_prepare_index_f32")
        return self._owned(blob), N

    def knn_prepare_columns(self, feats, cols, half=False, want_index=True):
        """feats [768, S] fp32 (packed encoder features), cols [N] int64 columns into it -> (prepared blob, N, index [1, 768, N] or None):
        the blob knn_prepare makes of feats[:, cols] (of its .half() with half=True), gathered in one launch
        (tvc_knn_prepare_index_cols_f32 / _f16); index = the selected vectors themselves, fp32 or fp16.  `cols` must lie in [0, S)
        (feature_retrieval.index_columns checks its plan on the host)."""
        feats = _prep(feats, "feats", self.device)
        if feats.dim() != 2 or feats.shape[0] != spec.SSL_DIM:
            raise ValueError(f"feats must be [768, S], got {tuple(feats.shape)}")
        cols = cols.to(device=self.device, dtype=torch.int64).contiguous()
        if cols.dim() != 1:
            raise ValueError("cols must be a 1-D list of columns")
        S, N = feats.shape[1], cols.numel()
        if N < 1:
            raise ValueError("cols selects no vector")
        index = torch.empty(1, spec.SSL_DIM, N, dtype=torch.float16 if half else _F32, device=self.device) if want_index else None
        if half:
            blob = torch.empty(self.lib.tvc_knn_prepared_elems_f16(N), dtype=_F32, device=self.device)
            self._ok(self.lib.tvc_knn_prepare_index_cols_f16(self.ctx, self._stream(), _ptr(feats), S, _ptr(cols), N, _ptr(blob), _ptr(index)),
                     "tvc_knn_prepare_index_cols_f16")
        else:
            blob = torch.empty(self.lib.tvc_knn_prepared_elems(N), dtype=_F32, device=self.device)
            self._ok(self.lib.tvc_knn_prepare_index_cols_f32(self.ctx, self._stream(), _ptr(feats), S, _ptr(cols), N, _ptr(blob), _ptr(index)),
                     "tvc_knn_prepare_index_cols_f32")
        return self._owned(blob), N, index

    def encode_ragged(self, wav, lengths):
        """wav [B, Lmax] (row b holds an utterance of lengths[b] samples, a multiple of 480, zero-padded behind it) -> (ssl [768, S],
        f0 [S], pre [B + 1]): every utterance encoded over its OWN length in one call (tvc_encode_ragged_f32), packed as one long
        utterance - utterance b owns columns pre[b] .. pre[b + 1], bit-identical to stft_mag + encoder on it alone."""
        wav, B, Lmax = self._rows(wav, ragged=True)
        lens = self._lens(lengths, B)
        p, n = self._query_ws("tvc_workspace_bytes_encode_ragged", B, Lmax, lens)
        pre = [0]
        for length in lengths:
            pre.append(pre[-1] + int(length) // spec.HOP)
        ssl = torch.empty(spec.SSL_DIM, pre[-1], dtype=_F32, device=self.device)
        f0 = torch.empty(pre[-1], dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_encode_ragged_f32(self.ctx, self._stream(), _ptr(wav), Lmax, lens, _ptr(ssl), _ptr(f0), B, p, n), "tvc_encode_ragged_f32")
        return ssl, f0, pre

    def _owned(self, blob):
        """The library remembers a prepared blob's N by device address (api.hip: blob_check) and asks for tvc_knn_forget before the
        memory is reused: the allocator recycles addresses, and a blob copied to where a blob of another size once lived must not
        inherit that record (it was refused as "prepared for N = 300, the call says N = 600").  The record goes when the tensor
        does; dropping it early only costs the next use one header read."""
        weakref.finalize(blob, _forget_blob, weakref.ref(self), blob.data_ptr()).atexit = False
        return blob

    # ---- the index of a call: shared (one blob), table (one per row), blend (M weighted per row), auto (table or blend + target registers) ----
    def _table(self, prepared, Ns, B):
        """(blob tensors, Ns) of B rows -> host arrays (void* [B], int64 [B]); the blobs must be 1-D float tensors on this device."""
        prepared, Ns = list(prepared), [int(n) for n in Ns]
        if len(prepared) != B or len(Ns) != B:
            raise ValueError(f"one prepared index and one N per row: got {len(prepared)} blobs and {len(Ns)} sizes for {B} rows")
        for b, t in enumerate(prepared):
            _check_dev(t, f"prepared[{b}]", self.device)
        return (ctypes.c_void_p * B)(*[t.data_ptr() for t in prepared]), (ctypes.c_int64 * B)(*Ns)

    def _blend_args(self, prepared, Ns, weights, B):
        """(flat row-major [B * M] blob tensors and sizes, weights [B, M]) -> (void* [B * M], int64 [B * M], M).  The weights stay where they
        are: a contiguous fp32 [B, M] tensor on this device that the kernels read when they run (so a captured graph follows in-place
        changes) - anything else is refused here, never copied."""
        _check_dev(weights, "weights", self.device)
        if weights.dim() != 2 or weights.shape[0] != B or weights.dtype != _F32 or not weights.is_contiguous():
            raise ValueError(f"weights must be a contiguous fp32 [B = {B}, M] tensor on the device, got {tuple(weights.shape)} {weights.dtype}")
        M = weights.shape[1]
        if not 1 <= M <= spec.BLEND_MAX:
            raise ValueError(f"a blend takes 1 ... {spec.BLEND_MAX} terms per row, got {M}")
        blobs, ns = self._table(prepared, Ns, B * M)
        return blobs, ns, M

    def _per_row(self, t, name, B):
        """a value per row of a call (`name`: target_f0, the target registers; alpha, the source's share; protect, its rise on unvoiced frames): a contiguous fp32 [B] tensor on
        this device, used in place (the kernels read it when they run) - anything else is refused here, never copied"""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor on the device (a contiguous fp32 [B = {B}]), got {type(t).__name__}")
        _check_dev(t, name, self.device)
        if t.dtype != _F32 or t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 [B = {B}] tensor on the device, got {tuple(t.shape)} {t.dtype}")
        return t

    def _neighbours(self, t, B):
        """k per row of a weighted call: a contiguous int32 [B] tensor on this device, used in place (the kernel clamps it to 1 .. 4 when it runs)"""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"neighbours must be a torch.Tensor on the device (a contiguous int32 [B = {B}]), got {type(t).__name__}")
        _check_dev(t, "neighbours", self.device)
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
            raise ValueError(f"neighbours must be a contiguous int32 [B = {B}] tensor on the device, got {tuple(t.shape)} {t.dtype}")
        return t

    def _weight_args(self, neighbours, width, B):
        """the weighted match's share of a call under the C parameters' names: either may be None (4 neighbours, an infinite width)"""
        return dict(neighbours=_ptr(self._neighbours(neighbours, B)) if neighbours is not None else None,
                    width=_ptr(self._per_row(width, "width", B)) if width is not None else None)

    def _index_args(self, form, prepared, Ns, weights, B):
        """The index of a call, checked on the host -> (what the entry takes for it, what its workspace query takes for it), each under
        the C parameters' names.  shared: (prepared, Ns) = one blob and its N; table: one blob and N per row; blend: weights [B, M] on the
        device, prepared / Ns row-major [B * M]; auto, track, alpha, protect, path: the blend form, or with weights None the table form
        as M = 1."""
        if form == "shared":
            return dict(prepared=_ptr(prepared), N=Ns), dict(N=int(max(Ns, 4)))
        if form == "table":
            blobs, ns = self._table(prepared, Ns, B)
            return dict(prepared=blobs, N=ns), dict(N=ns)
        if form in ("auto", "track", "alpha", "protect", "path", "tuned", "weighted", "joined") and weights is None:
            blobs, ns = self._table(prepared, Ns, B)
            return dict(prepared=blobs, N=ns, M=1, weights=None), dict(N=ns, M=1)
        blobs, ns, M = self._blend_args(prepared, Ns, weights, B)
        return dict(prepared=blobs, N=ns, M=M, weights=_ptr(weights)), dict(N=ns, M=M)

    @staticmethod
    def _lens(lengths, B):
        """one length per row -> int64 [B] on the host"""
        if len(lengths) != B:
            raise ValueError(f"lengths: {len(lengths)} entries for {B} rows")
        return (ctypes.c_int64 * B)(*[int(x) for x in lengths])

    def _rows(self, wav, ragged=False):
        """what every convert* / encode_ragged does with its input first: wav [B, L] fp32 on this device, L in whole frames -> (wav, B, L)"""
        wav = _prep(wav, "wave", self.device)
        B, L = wav.shape
        if L % spec.HOP:
            raise ValueError("the padded length must be a multiple of 480" if ragged else "waveform length must be a multiple of 480 (autopad_waveform)")
        return wav, B, L

    # ---- kNN match: one driver, the public forms forward to it ----
    def _match(self, form, src, prepared, Ns, weights=None, want_indices=False, alpha=None, f0=None, protect=None, neighbours=None, width=None,
               want_similarities=False, join=None, want_anchors=False, want_affinities=False):
        """src [B, 768, T] matched against the index (`form`, prepared, Ns, weights: _index_args) -> matched [B, 768, T] (, indices [B, T, 4];
        [M, B, T, 4] for a blend: each term's own search).  form "alpha": the table (weights None) or blend form, and out = matched *
        (1 - alpha[b]) + src * alpha[b] (alpha: _per_row; indices always [M, B, T, 4]).  form "protect": the alpha form with the frame's share
        a_t = a + (1 - a) * (protect[b] * w[t]) in alpha's place, w from f0 [B, 1, T] / [B, T] (alpha None: a = 0).  form "weighted": the
        protect form with alpha, protect and f0 all optional and neighbours / width (_weight_args) behind them (, similarities [M, B, T, 4]).
        form "joined": the weighted form with join (_per_row: the continuity weight) behind width (, anchors [M, B, T] int32, affinities
        [M, B, T, 4, 4])."""
        src = _prep(src, "source", self.device)
        B, C, T = src.shape
        if C != spec.SSL_DIM:
            raise ValueError(f"source must have {spec.SSL_DIM} channels")
        named, sized = self._index_args(form, prepared, Ns, weights, B)
        named.update(src=_ptr(src), B=B, T=T)
        if form == "alpha":
            named["alpha"] = _ptr(self._per_row(alpha, "alpha", B))
        elif form == "protect":
            f0 = _prep(f0, "f0", self.device)
            if f0.numel() != B * T or f0.shape[0] != B:
                raise ValueError(f"f0 must hold one value per frame, [B = {B}, 1, T = {T}] or [B, T], got {tuple(f0.shape)}")
            named["alpha"] = _ptr(self._per_row(alpha, "alpha", B)) if alpha is not None else None
            named["protect"] = _ptr(self._per_row(protect, "protect", B))
            named["f0"] = _ptr(f0)
        elif form in ("weighted", "joined"):
            if protect is not None:
                f0 = _prep(f0, "f0", self.device)
                if f0.numel() != B * T or f0.shape[0] != B:
                    raise ValueError(f"f0 must hold one value per frame, [B = {B}, 1, T = {T}] or [B, T], got {tuple(f0.shape)}")
            named["alpha"] = _ptr(self._per_row(alpha, "alpha", B)) if alpha is not None else None
            named["protect"] = _ptr(self._per_row(protect, "protect", B)) if protect is not None else None
            named["f0"] = _ptr(f0) if protect is not None else None
            named.update(self._weight_args(neighbours, width, B))
            if form == "joined":
                named["join"] = _ptr(self._per_row(join, "join", B))
        out = torch.empty_like(src)
        terms = (sized["M"],) if "M" in sized else ()      # a blend's terms
        idx = torch.empty(*terms, B, T, 4, dtype=torch.int64, device=self.device) if want_indices else None
        sims = torch.empty(*terms, B, T, 4, dtype=_F32, device=self.device) if want_similarities else None
        query, entry = _names(form)
        named["ws"], named["ws_bytes"] = self._query_ws(query, B=B, L=T * spec.HOP, **sized)
        named.update(ctx=self.ctx, stream=self._stream(), out=_ptr(out), idx_out=_ptr(idx))
        if form in ("weighted", "joined"):
            named["sims_out"] = _ptr(sims)
        anchors = torch.empty(*terms, B, T, dtype=torch.int32, device=self.device) if want_anchors else None
        aff = torch.empty(*terms, B, T, 4, 4, dtype=_F32, device=self.device) if want_affinities else None
        if form == "joined":
            named.update(anchor_out=_ptr(anchors), affinity_out=_ptr(aff))
        self._ok(getattr(self.lib, entry)(*_lib.arguments(entry, named)), entry)
        res = (out,) + ((idx,) if want_indices else ()) + ((sims,) if want_similarities else ()) + ((anchors,) if want_anchors else ()) + ((aff,) if want_affinities else ())
        return res if len(res) > 1 else out

    def knn_match(self, src, prepared, N, want_indices=False):
        return self._match("shared", src, prepared, N, None, want_indices)

    def knn_match_multi(self, src, prepared, Ns, want_indices=False):
        """src [B, 768, T]; row b searches prepared[b] (a blob of knn_prepare, Ns[b] vectors) -> matched [B, 768, T] (, indices [B, T, 4]):
        one call, every row equal to its own knn_match."""
        return self._match("table", src, prepared, Ns, None, want_indices)

    def knn_match_blend(self, src, prepared, Ns, weights, want_indices=False):
        """src [B, 768, T]; term m of row b is prepared[b * M + m] (Ns likewise), weights [B, M] on the device -> matched [B, 768, T] =
        w_0 * match_0 + w_1 * match_1 + ... in term order (, indices [M, B, T, 4]: each term's own search): tvc_knn_match_blend_f32."""
        return self._match("blend", src, prepared, Ns, weights, want_indices)

    def knn_match_alpha(self, src, prepared, Ns, alpha, weights=None, want_indices=False):
        """knn_match_multi (weights None: prepared / Ns one per row) or knn_match_blend (weights [B, M]) keeping a share of the source:
        out = matched * (1 - alpha[b]) + src * alpha[b], three separate fp32 roundings, alpha a contiguous fp32 [B] device tensor read when
        the kernel runs (, indices [M, B, T, 4], M = 1 without weights: what the alpha-less call finds): tvc_knn_match_alpha_f32."""
        return self._match("alpha", src, prepared, Ns, weights, want_indices, alpha)

    def knn_match_protect(self, src, f0, prepared, Ns, alpha, protect, weights=None, want_indices=False):
        """knn_match_alpha with a share per FRAME: a_t = a + (1 - a) * (protect[b] * w[t]), w[t] = 1 - (u[t-1] + 2 u[t] + u[t+1]) / 4 the
        unvoiced weight of frame t from f0 [B, 1, T] / [B, T] (u = f0 > 0, edges repeated, rows apart), alpha / protect contiguous fp32 [B]
        device tensors read when the kernels run (alpha None: a = 0): tvc_knn_match_protect_f32."""
        return self._match("protect", src, prepared, Ns, weights, want_indices, alpha, f0, protect)

    def knn_match_weighted(self, src, prepared, Ns, neighbours=None, width=None, weights=None, alpha=None, f0=None, protect=None, want_indices=False,
                           want_similarities=False):
        """knn_match_multi / _blend / _alpha / _protect (weights, alpha, protect and its f0 all optional) with the mean over the k nearest of
        the four rows, each weighted by w_e = clamp(1 - (s_0 - s_e) / width, 0, 1): neighbours a contiguous int32 [B] device tensor (k,
        clamped to 1 .. 4; None: 4), width a contiguous fp32 [B] device tensor in cosine units (None: +inf), both read when the kernel runs
        (, indices [M, B, T, 4], similarities [M, B, T, 4]: what the lists held when the weights were formed): tvc_knn_match_weighted_f32;
        the definition is in include/tinyvc_hip.h."""
        return self._match("weighted", src, prepared, Ns, weights, want_indices, alpha, f0, protect, neighbours, width, want_similarities)

    def knn_match_joined(self, src, prepared, Ns, join, neighbours=None, width=None, weights=None, alpha=None, f0=None, protect=None, want_indices=False,
                         want_similarities=False, want_anchors=False, want_affinities=False):
        """knn_match_weighted along a path: join a contiguous fp32 [B] device tensor, the continuity weight c of every row, read when the
        kernels run - the weights form around the neighbour that a Viterbi path over the row's frames chose, a neighbour gaining by its
        similarity to the query and by c times its cosine to the neighbour chosen for the frame before (, indices, similarities, anchors
        [M, B, T] int32: the path, affinities [M, B, T, 4, 4]: the cosines between neighbouring frames' rows, frame 0's zeros):
        tvc_knn_match_joined_f32; the definition is in include/tinyvc_hip.h."""
        return self._match("joined", src, prepared, Ns, weights, want_indices, alpha, f0, protect, neighbours, width, want_similarities, join, want_anchors,
                           want_affinities)

    def frame_share(self, f0_packed, start, counts, alpha, protect):
        """The per-frame share alone (tvc_frame_share_f32): f0_packed any contiguous fp32 device tensor, row i = its flattened values
        [start[i], start[i] + counts[i]); alpha (or None = 0) / protect contiguous fp32 [rows] device tensors -> a tensor like f0_packed
        holding a_t at every row's columns and zeros elsewhere."""
        f0 = _prep(f0_packed, "f0", self.device)
        start, counts = [int(x) for x in start], [int(x) for x in counts]
        rows = len(start)
        if rows < 1 or len(counts) != rows or any(a < 0 or c < 0 or a + c > f0.numel() for a, c in zip(start, counts)):
            raise ValueError(f"frame_share: start and counts must be equally many rows within the {f0.numel()} values of f0")
        al = self._per_row(alpha, "alpha", rows) if alpha is not None else None
        pr = self._per_row(protect, "protect", rows)
        out = torch.zeros_like(f0)
        I64 = ctypes.c_int64 * rows
        self._ok(self.lib.tvc_frame_share_f32(self.ctx, self._stream(), _ptr(f0), I64(*start), I64(*counts), rows, _ptr(al), _ptr(pr), _ptr(out)),
                 "tvc_frame_share_f32")
        return out

    # ---- convert: one driver, the eight public forms forward to it ----
    def _track_args(self, track, S, T):
        """a PitchTrack's share of a call over S streams of T frames, checked on the host, under the C parameters' names (and in their order)"""
        if track.n_streams != S:
            raise ValueError(f"track: a tracker of {track.n_streams} streams for {S} rows")
        start, n = track.columns(T)
        state = checked(track, TRACK_STATE, S, self.device, "track.")      # the kernel indexes the state by (S, W): never past it
        return _TrackArgs(start, n, track.window_frames, track.min_voiced, track.slew, *map(_ptr, state))

    def _carry_args(self, carry, S, T):
        """a PitchCarry's share of a call over S streams of T frames, checked on the host, under the C parameters' names"""
        if carry.n_streams != S:
            raise ValueError(f"carry: a carry of {carry.n_streams} streams for {S} rows")
        if T <= carry.hop_frames:
            raise ValueError(f"carry: hop_frames = {carry.hop_frames} must be below the call's T = {T} frames (frame hop_frames is the next window's first)")
        state = checked(carry, CARRY_STATE, S, self.device, "carry.")      # the kernel indexes the state by (S, 512): never past it
        return _CarryArgs(carry.hop_frames, *map(_ptr, state))

    def _snap_tensors(self, tune, rows, what):
        """a PitchSnap's table and strengths as the kernel reads them, bound to this device and `rows` rows and checked: (notes, strength)"""
        tune.bind(self.device, rows)
        for t, name, shape in ((tune.notes, "notes", (128,)), (tune.strength, "strength", (rows,))):
            _check_dev(t, f"{what}.{name}", self.device)
            if t.dtype != _F32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what}.{name} must be a contiguous fp32 {list(shape)} tensor, got {t.dtype} {tuple(t.shape)}")
        return tune.notes, tune.strength

    def _snap_args(self, tune, tune_carry, B, T):
        """a PitchSnap's (and its SnapCarry's) share of a call over B rows of at most T frames, checked on the host, under the C parameters' names"""
        notes, strength = self._snap_tensors(tune, B, "tune")
        state = (0, None, None)
        if tune_carry is not None:
            if tune_carry.n_streams != B:
                raise ValueError(f"tune_carry: a carry of {tune_carry.n_streams} streams for {B} rows")
            if T < tune_carry.hop_frames:
                raise ValueError(f"tune_carry: hop_frames = {tune_carry.hop_frames} must be at most the call's T = {T} frames")
            state = (tune_carry.hop_frames, *map(_ptr, checked(tune_carry, SNAP_STATE, B, self.device, "tune_carry.")))      # the kernel indexes the state by row: never past it
        return _SnapArgs(ctypes.byref(tune.settings()), _ptr(notes), _ptr(strength), *state)

    def _convert(self, form, wav, prepared, Ns, pitch_shift, noise_angle=None, lengths=None, weights=None, target_f0=None, out=None, shift_out=None,
                 track=None, alpha=None, protect=None, path=None, carry=None, tune=None, tune_carry=None, neighbours=None, width=None, join=None):
        """wav [B, L] converted toward the index (`form`, prepared, Ns, weights: _index_args) -> wave [B, L]; form "auto" / "track" ->
        (wave, shifts [B]).  "track": "auto" with the register taken from `track` (a PitchTrack: the streams' history), equal lengths only.
        "alpha": the table / blend call keeping the share alpha[b] of row b's own content features (alpha: _per_row); with target_f0 it is the
        "auto" call (-> (wave, shifts)), with `track` as well the "track" call.  "protect": the "alpha" call with protect[b] (_per_row) behind
        alpha, which may then be None (a = 0): the share rises to a + (1 - a) * protect[b] on the unvoiced frames of the f0 the call decodes.
        "path": the "protect" call (alpha and protect may both be None) with `path`, a PitchPath, behind protect: f0 is the Viterbi decode of the
        call's own logits over each utterance, and everything behind the encoder reads that one.  `carry` (with "path", equal lengths only): a
        PitchCarry of B streams - row b's decode starts from carry.scores[b] and leaves the best-predecessor values of frame carry.hop_frames
        there, in place (tvc_convert_carry_f32).  "tuned": the "path" call with alpha, protect, path and carry ALL optional and `tune`, a
        PitchSnap, behind them: the f0 the decoder reads is snapped to tune.notes in place, one launch in front of the decoder
        (tvc_tuned_convert_f32 / tvc_tuned_convert_ragged_f32); `tune_carry` (equal lengths only): a SnapCarry of B streams, read at frame 0 and
        written behind frame tune_carry.hop_frames - 1.  "weighted": the "tuned" call with `tune` optional too and neighbours / width
        (_weight_args: k and the similarity width per row, either may be None) behind protect: the match is the weighted mean over the k
        nearest rows (tvc_weighted_convert_f32 / tvc_weighted_convert_ragged_f32; the workspace is the tuned call's).  "joined": the "weighted"
        call with join (_per_row: the continuity weight per row) behind width - the match along a path (tvc_joined_convert_f32 /
        tvc_joined_convert_ragged_f32, queries of their own).
        lengths: a ragged batch (row b holds an utterance of lengths[b] samples, a multiple of 480, zero-padded behind it; every utterance
        is converted over its OWN length).  pitch_shift: a float, or one per row for every form but "shared".  Every host check comes
        first, then the noise draw (which advances torch's generator), then device work: a refused call leaves no trace.
        Every value is computed once, under the name of the C parameter it is for (a feature the call lacks keeps its "off" value); the
        entry takes the ones it declares (_lib.arguments)."""
        ragged = lengths is not None
        wav, B, L = self._rows(wav, ragged)
        T = L // spec.HOP
        named = dict(_FEATURES_OFF, wav=_ptr(wav), B=B)
        named["Lmax" if ragged else "L"] = L
        if ragged:
            named["lens"] = self._lens(lengths, B)
        index, sized = self._index_args(form, prepared, Ns, weights, B)
        named.update(index)
        if form == "shared":
            named["prepared_index"] = named.pop("prepared")      # the conversion's name for the stage call's `prepared`
        if ragged and (form == "track" or track is not None):
            raise ValueError("track: streams advance in lock step, there is no ragged form")
        if carry is not None and (form not in ("path", "tuned", "weighted", "joined") or path is None or ragged):
            raise ValueError("carry: the pitch path's state - it goes with form \"path\", and streams advance in lock step: there is no ragged form")
        found = form in ("auto", "track")      # the shifts are found on the device: pitch_shift is the offset, the applied shifts come back
        if (form not in ("weighted", "joined") and (tune is None) != (form != "tuned")) or (tune_carry is not None and (tune is None or ragged)):
            raise ValueError("tune goes with form \"tuned\" (and tune_carry with tune; streams advance in lock step: there is no ragged form)")
        shares = form in ("alpha", "protect", "path", "tuned", "weighted", "joined")      # the table / blend call with or without target registers (and, equal lengths, a tracker), plus the source's share
        if shares:
            found = target_f0 is not None
            if track is not None and not found:
                raise ValueError("track needs target_f0: the tracker finds the register the automatic shift starts from")
            if form == "alpha" or alpha is not None:
                named["alpha"] = _ptr(self._per_row(alpha, "alpha", B))
            if form == "protect" or (form in ("path", "tuned", "weighted", "joined") and protect is not None):
                named["protect"] = _ptr(self._per_row(protect, "protect", B))
            if form in ("weighted", "joined"):
                named.update(self._weight_args(neighbours, width, B))
            if form == "joined":
                named["join"] = _ptr(self._per_row(join, "join", B))
            if form == "path" or (form in ("tuned", "weighted", "joined") and path is not None):
                named["path"] = ctypes.byref(path.settings())
                if carry is not None:
                    named.update(self._carry_args(carry, B, T)._asdict())
            if form == "tuned" or (form in ("weighted", "joined") and tune is not None):
                named.update(self._snap_args(tune, tune_carry, B, T)._asdict())
        if found:
            named["target_f0"] = _ptr(self._per_row(target_f0, "target_f0", B))
        if form == "track" or (shares and track is not None):
            named.update(self._track_args(track, B, T)._asdict())
        named["pitch_shift"], shifts = pitch_shifts(pitch_shift, B)
        if form == "shared" and shifts is not None:
            raise ValueError("pitch_shift: one shared index takes one shift (a shift per row takes an index per row)")
        named["pitch_shifts"] = _floats(shifts)
        a, named["seed"] = self._angle(noise_angle, B, T)
        wave = out if out is not None else torch.empty(B, L, dtype=_F32, device=self.device)
        if found:
            sh = shift_out if shift_out is not None else torch.empty(B, dtype=_F32, device=self.device)
            named["shift_out"] = _ptr(sh)
        query, entry = _names(form, "carry" if carry is not None and form == "path" else ragged)
        named["ws"], named["ws_bytes"] = self._query_ws(query, B=B, lens=named["lens"], **{"Lmax" if ragged else "L": L}, **sized)
        named.update(ctx=self.ctx, stream=self._stream(), noise_angle=_ptr(a), wave=_ptr(wave))
        self._ok(getattr(self.lib, entry)(*_lib.arguments(entry, named)), entry)
        return (wave, sh) if found else wave

    def convert(self, wav, prepared, N, pitch_shift, noise_angle=None, out=None):
        return self._convert("shared", wav, prepared, N, pitch_shift, noise_angle, out=out)

    def convert_ragged(self, wav, lengths, prepared, N, pitch_shift, noise_angle=None):
        """wav [B, Lmax] (row b holds an utterance of lengths[b] samples, a multiple of 480, zero-padded behind it) -> [B, Lmax]:
        every utterance converted over its OWN length (tvc_convert_ragged_f32: per-utterance lengths inside the kernels)."""
        return self._convert("shared", wav, prepared, N, pitch_shift, noise_angle, lengths)

    def convert_multi(self, wav, prepared, Ns, pitch_shift, noise_angle=None, out=None):
        """convert with one prepared index per row (and pitch_shift a float or one per row): tvc_convert_multi_f32."""
        return self._convert("table", wav, prepared, Ns, pitch_shift, noise_angle, out=out)

    def convert_ragged_multi(self, wav, lengths, prepared, Ns, pitch_shift, noise_angle=None):
        """convert_ragged with one prepared index per row (and pitch_shift a float or one per row): tvc_convert_ragged_multi_f32."""
        return self._convert("table", wav, prepared, Ns, pitch_shift, noise_angle, lengths)

    def convert_blend(self, wav, prepared, Ns, weights, pitch_shift, noise_angle=None, out=None):
        """convert toward a weighted blend of M prepared indices per row (pitch_shift a float or one per row): tvc_convert_blend_f32."""
        return self._convert("blend", wav, prepared, Ns, pitch_shift, noise_angle, weights=weights, out=out)

    def convert_ragged_blend(self, wav, lengths, prepared, Ns, weights, pitch_shift, noise_angle=None):
        """convert_ragged toward a weighted blend of M prepared indices per row: tvc_convert_ragged_blend_f32."""
        return self._convert("blend", wav, prepared, Ns, pitch_shift, noise_angle, lengths, weights)

    def convert_auto(self, wav, prepared, Ns, target_f0, pitch_shift=0.0, weights=None, noise_angle=None, out=None, shift_out=None):
        """convert_multi (weights None: one prepared index per row) or convert_blend (weights [B, M] on the device, prepared / Ns [B * M]) with the
        shift found on the device: row b is shifted by pitch_shift (a float or one per row, now the offset) + 12 log2(target_f0[b] / the
        lower median of the row's own voiced f0) -> (wave [B, L], shifts [B] on the device): tvc_convert_auto_f32."""
        return self._convert("auto", wav, prepared, Ns, pitch_shift, noise_angle, None, weights, target_f0, out, shift_out)

    def convert_ragged_auto(self, wav, lengths, prepared, Ns, target_f0, pitch_shift=0.0, weights=None, noise_angle=None):
        """convert_auto over a ragged batch (every utterance's register is the median over its OWN frames): tvc_convert_ragged_auto_f32."""
        return self._convert("auto", wav, prepared, Ns, pitch_shift, noise_angle, lengths, weights, target_f0)

    # ---- the pitch path: a Viterbi decode of rows of logits (tvc_pitch_path_f32) ----
    def _carry_rows(self, t, name, rows):
        """prior / carry_out of pitch_path as the kernel indexes it: a contiguous fp32 [rows, 512] tensor on the device, used in place"""
        _check_dev(t, name, self.device)
        if t.dtype != _F32 or tuple(t.shape) != (rows, spec.PITCH_CLASSES) or not t.is_contiguous():
            raise ValueError(f"pitch_path: {name} must be a contiguous fp32 [rows = {rows}, {spec.PITCH_CLASSES}] tensor, got {t.dtype} {tuple(t.shape)}")
        return t

    def pitch_path(self, logits, settings, row_start=None, pitch_shift=0.0, want_shifted=False, prior=None, carry_out=None, carry_frame=0):
        """The pitch path of rows of logits (include/tinyvc_hip.h has the definition; `settings` a PitchPath): logits [B, 512, T] (every row
        a run of T columns), or a packed [512, Ttot] / [1, 512, Ttot] with row_start = rows + 1 ascending column numbers (row b =
        columns [row_start[b], row_start[b + 1])) -> (f0 [B, 1, T] or [1, 1, Ttot] fp32, path int32 of f0's shape, scores [rows, 512] = the
        last frame's normalised scores[, f0 shifted by pitch_shift - a float or one per row - when want_shifted]).  Columns outside every
        row are 0.  The carry (tvc_pitch_path_carry_f32): `prior` [rows, 512] is added, sanitised, to each row's first emissions, and
        `carry_out` [rows, 512] receives the best-predecessor values of frame `carry_frame` >= 1, which every non-empty row must have;
        contiguous fp32 device tensors used in place, either alone, or one tensor as both.  Neither is the call as it was."""
        lg = _prep(logits, "logits", self.device)
        if lg.dim() == 2:
            lg = lg[None]
        if lg.dim() != 3 or lg.shape[1] != spec.PITCH_CLASSES or lg.shape[2] < 1:
            raise ValueError(f"pitch_path: logits [B, {spec.PITCH_CLASSES}, T] or a packed [{spec.PITCH_CLASSES}, Ttot], got {tuple(lg.shape)}")
        B, _, T = lg.shape
        if row_start is None:
            row_start = [b * T for b in range(B + 1)]
        elif B != 1:
            raise ValueError("pitch_path: row_start goes with a packed [512, Ttot]")
        row_start = [int(x) for x in row_start]
        rows = len(row_start) - 1
        if rows < 1 or row_start[0] < 0 or row_start[-1] > B * T or any(a > b for a, b in zip(row_start, row_start[1:])):
            raise ValueError(f"pitch_path: row_start must be rows + 1 ascending column numbers within the {B * T} columns of logits")
        shift, shifts = pitch_shifts(pitch_shift, rows)
        I64 = ctypes.c_int64 * rows
        start, count = I64(*row_start[:-1]), I64(*(b - a for a, b in zip(row_start, row_start[1:])))
        carried = ()
        if prior is not None or carry_out is not None:
            h = integer(carry_frame, "pitch_path", "carry_frame") if carry_out is not None else 0
            if carry_out is not None and (h < 1 or any(0 < n <= h for n in count)):
                raise ValueError(f"pitch_path: carry_frame = {h} must be >= 1 and every non-empty row must have more frames (rows of {sorted(set(count))})")
            carried = (h, _ptr(self._carry_rows(prior, "prior", rows)) if prior is not None else None,
                       _ptr(self._carry_rows(carry_out, "carry_out", rows)) if carry_out is not None else None)
        f0 = torch.zeros(B, 1, T, dtype=_F32, device=self.device)
        path = torch.zeros(B, 1, T, dtype=torch.int32, device=self.device)
        scores = torch.zeros(rows, spec.PITCH_CLASSES, dtype=_F32, device=self.device)
        out = torch.zeros_like(f0) if want_shifted else None
        p, n = self._query_ws("tvc_workspace_bytes_pitch_path", start, count, rows)
        entry = "tvc_pitch_path_carry_f32" if carried else "tvc_pitch_path_f32"
        self._ok(getattr(self.lib, entry)(self.ctx, self._stream(), _ptr(lg), start, count, rows, T, ctypes.byref(settings.settings()), *carried, shift,
                                          _floats(shifts), _ptr(f0), _ptr(out), _ptr(path), _ptr(scores), p, n), entry)
        return (f0, path, scores, out) if want_shifted else (f0, path, scores)

    # ---- pitch correction: rows of f0 snapped to a table of notes (tvc_pitch_snap_f32) ----
    def pitch_snap(self, f0, tune, row_start=None, row_count=None, carry=None, in_place=False):
        """The pitch correction of rows of f0 (include/tinyvc_hip.h has the definition; `tune` a PitchSnap, whose notes [128] and strength
        [rows] are read on the device when the kernel runs): f0 [B, 1, T] / [B, T] (every row a run of T columns), or any contiguous f0 with
        row_start (and row_count; default: up to the next row's start, row_start then has rows + 1 entries) naming the rows' columns in the
        flattened f0 -> (out like f0 - f0 itself with in_place -, note_out int32 like f0: the note of every frame, -1 for a frame that passed
        untouched).  Columns outside every row keep f0's value and note -1.  `carry`: a SnapCarry of `rows` streams, read at every row's
        first frame and written behind frame carry.hop_frames - 1, which every non-empty row must have."""
        f0 = _prep(f0, "f0", self.device)
        if row_start is None:
            if f0.dim() < 2:
                raise ValueError("pitch_snap: f0 [B, 1, T] or [B, T], or row_start for a packed f0")
            rows, T = f0.shape[0], f0.numel() // max(f0.shape[0], 1)
            row_start, row_count = [b * T for b in range(rows)], [T] * rows
        row_start = [int(x) for x in row_start]
        if row_count is None:
            row_start, row_count = row_start[:-1], [b - a for a, b in zip(row_start, row_start[1:])]
        row_count = [int(x) for x in row_count]
        rows, end = len(row_start), 0
        if rows < 1 or len(row_count) != rows:
            raise ValueError("pitch_snap: row_start and row_count must name the same rows, at least one")
        for a, n in zip(row_start, row_count):
            if a < end or n < 0 or a + n > f0.numel():
                raise ValueError(f"pitch_snap: the rows must be ascending and apart within the {f0.numel()} values of f0")
            end = a + n
        notes, strength = self._snap_tensors(tune, rows, "tune")
        state = (0, None, None)
        if carry is not None:
            if carry.n_streams != rows:
                raise ValueError(f"pitch_snap: a carry of {carry.n_streams} streams for {rows} rows")
            if any(0 < n < carry.hop_frames for n in row_count):
                raise ValueError(f"pitch_snap: every non-empty row needs at least carry.hop_frames = {carry.hop_frames} frames (rows of {sorted(set(row_count))})")
            state = (carry.hop_frames, *map(_ptr, checked(carry, SNAP_STATE, rows, self.device, "carry.")))
        out = f0 if in_place else f0.clone()
        note_out = torch.full(f0.shape, -1, dtype=torch.int32, device=self.device)
        I64 = ctypes.c_int64 * rows
        self._ok(self.lib.tvc_pitch_snap_f32(self.ctx, self._stream(), _ptr(f0), I64(*row_start), I64(*row_count), rows, ctypes.byref(tune.settings()), _ptr(notes),
                                             _ptr(strength), *state, _ptr(out), _ptr(note_out)), "tvc_pitch_snap_f32")
        return out, note_out

    # ---- the pitch register of rows of f0, and the shift onto a target's (tvc_pitch_match_f32) ----
    def pitch_match(self, f0, row_start=None, target_f0=None, pitch_shift=0.0, want_shifted=False):
        """The pitch register of rows of f0, and the shift onto a target's: f0 [B, 1, T] / [B, T] (every row a run of T columns), or any
        contiguous f0 with row_start = rows + 1 ascending column numbers (row b = [row_start[b], row_start[b + 1]) of the flattened f0) ->
        (median [rows] fp32 - the lower median of the values > 0, 0 without one -, voiced [rows] int32, shift [rows] fp32 =
        pitch_shift (a float or one per row) + 12 log2(target_f0 / median), f0 shifted by it or None).  target_f0 (optional): a
        contiguous fp32 [rows] device tensor in Hz; without it the call measures and shift is the offset."""
        f0 = _prep(f0, "f0", self.device)
        if row_start is None:
            if f0.dim() < 2:
                raise ValueError("pitch_match: f0 [B, 1, T] or [B, T], or row_start for a packed f0")
            rows, T = f0.shape[0], f0.numel() // max(f0.shape[0], 1)
            row_start = [b * T for b in range(rows + 1)]
        row_start = [int(x) for x in row_start]
        rows = len(row_start) - 1
        if rows < 1 or row_start[0] < 0 or row_start[-1] > f0.numel() or any(a > b for a, b in zip(row_start, row_start[1:])):
            raise ValueError(f"pitch_match: row_start must be rows + 1 ascending column numbers within the {f0.numel()} values of f0")
        shift, shifts = pitch_shifts(pitch_shift, rows)
        tgt = self._per_row(target_f0, "target_f0", rows) if target_f0 is not None else None
        med = torch.empty(rows, dtype=_F32, device=self.device)
        voiced = torch.empty(rows, dtype=torch.int32, device=self.device)
        sh = torch.empty(rows, dtype=_F32, device=self.device)
        out = torch.zeros_like(f0) if want_shifted else None
        self._ok(self.lib.tvc_pitch_match_f32(self.ctx, self._stream(), _ptr(f0), (ctypes.c_int64 * (rows + 1))(*row_start), rows, _ptr(tgt), shift, _floats(shifts),
                                              _ptr(med), _ptr(voiced), _ptr(sh), _ptr(out)), "tvc_pitch_match_f32")
        return med, voiced, sh, out

    def pitch_track(self, f0, track, target_f0, pitch_shift=0.0, want_shifted=False):
        """One block of a PitchTrack over a caller's f0 [S, 1, T] / [S, T] (tvc_pitch_track_f32): the voiced frames among the tracked columns
        (track.columns(T)) enter each stream's ring, `track.auto` moves toward 12 log2(target_f0 / the ring's lower median) ->
        (median [S] fp32, count [S] int64, shift [S] fp32 = pitch_shift (a float or one per stream) + track.auto, f0 shifted by it or None).
        target_f0: a contiguous fp32 [S] device tensor in Hz.  The state in `track` is updated in place."""
        f0 = _prep(f0, "f0", self.device)
        if f0.dim() < 2:
            raise ValueError("pitch_track: f0 [S, 1, T] or [S, T]")
        S, T = f0.shape[0], f0.numel() // max(f0.shape[0], 1)
        targs = self._track_args(track, S, T)
        shift, shifts = pitch_shifts(pitch_shift, S)
        tgt = self._per_row(target_f0, "target_f0", S)
        med = torch.empty(S, dtype=_F32, device=self.device)
        cnt = torch.empty(S, dtype=torch.int64, device=self.device)
        sh = torch.empty(S, dtype=_F32, device=self.device)
        out = torch.empty_like(f0) if want_shifted else None
        start, n, W, min_voiced, slew, ring, count, auto = targs
        self._ok(self.lib.tvc_pitch_track_f32(self.ctx, self._stream(), _ptr(f0), S, T, start, n, _ptr(tgt), shift, _floats(shifts), W, min_voiced, slew,
                                              ring, count, auto, _ptr(med), _ptr(cnt), _ptr(sh), _ptr(out)), "tvc_pitch_track_f32")
        return med, cnt, sh, out

    # ---- index-sharded match (one prepared index shard per rank; merged by parallel.match_features_sharded) ----
    METRICS = {"cos": 0, "IP": 1, "L2": 2}

    def knn_match_general(self, src, index, k, metrics, want_indices=False):
        """match_features for any k in 1..8 and metrics in {'cos', 'IP', 'L2'} on the RAW index [768, N] (plain fp32, csrc/knn_general.hip):
        src [B, 768, T] -> matched [B, 768, T] (, indices [B, T, k] int64 in rank order)."""
        src = _prep(src, "source", self.device)
        index = _prep(index, "index", self.device)
        if metrics not in self.METRICS:
            raise ValueError(f"metrics must be one of {sorted(self.METRICS)}, got {metrics!r}")
        if index.dim() != 2 or index.shape[0] != spec.SSL_DIM or src.dim() != 3 or src.shape[1] != spec.SSL_DIM:
            raise ValueError("knn_match_general: src [B, 768, T], index [768, N]")
        B, _, T = src.shape
        N = index.shape[1]
        if not 1 <= int(k) <= 8:
            raise NotImplementedError("the HIP kernel serves k = 1 ... 8")
        if N < k:
            raise RuntimeError("selected index k out of range")      # what torch.topk raises in the reference
        out = torch.empty(B, spec.SSL_DIM, T, dtype=_F32, device=self.device)
        idx = torch.empty(B, T, int(k), dtype=torch.int64, device=self.device)
        self._ok(self.lib.tvc_knn_match_general_f32(self.ctx, self._stream(), _ptr(src), _ptr(index), N, int(k), self.METRICS[metrics], _ptr(out), _ptr(idx), None,
                                                    B, T, None, 0), "tvc_knn_match_general_f32")
        return (out, idx) if want_indices else out

    def knn_topk(self, src, prepared, N):
        """This shard's top-4 per query: (sims [B,T,4] fp32 descending, idx [B,T,4] int64 local indices)."""
        src = _prep(src, "source", self.device)
        B, C, T = src.shape
        if C != spec.SSL_DIM:
            raise ValueError(f"source must have {spec.SSL_DIM} channels")
        sims = torch.empty(B, T, 4, dtype=_F32, device=self.device)
        idx = torch.empty(B, T, 4, dtype=torch.int64, device=self.device)
        p, n = self._wsargs(B, T * spec.HOP, N)
        self._ok(self.lib.tvc_knn_topk_f32(self.ctx, self._stream(), _ptr(src), _ptr(prepared), N, _ptr(sims), _ptr(idx), B, T, p, n), "tvc_knn_topk_f32")
        return sims, idx

    def knn_gather_slots(self, prepared, N, idx):
        """idx [B,T,4] int64 local indices (negative = not on this shard) -> slots [B,T,4,768] raw rows / zeros."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        slots = torch.empty(*idx.shape, spec.SSL_DIM, dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_knn_gather_slots_f32(self.ctx, self._stream(), _ptr(prepared), N, _ptr(idx), _ptr(slots), idx.numel()), "tvc_knn_gather_slots_f32")
        return slots

    def knn_finish(self, slots):
        """slots [B,T,4,768] -> [B,768,T]: mean of the four rows in the single-GPU summation order."""
        slots = _prep(slots, "slots", self.device)
        B, T = slots.shape[0], slots.shape[1]
        out = torch.empty(B, spec.SSL_DIM, T, dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_knn_finish_f32(self.ctx, self._stream(), _ptr(slots), _ptr(out), B, T), "tvc_knn_finish_f32")
        return out

    # ---- compacting an index: k-means over a prepared blob (tvc_index_*_f32) ----
    def _compact_ws(self, N, K):
        return self._query_ws("tvc_workspace_bytes_index_compact", int(N), int(K))

    def index_assign(self, points_blob, N, cent_blob, K, assign=None):
        """Nearest centroid (cosine) of every raw vector of `points_blob` (a blob of knn_prepare, either kind, N vectors) among the K vectors of
        `cent_blob` (an fp32-kind blob) -> (assign [N] int64, sims [N] fp32, moved [1] int32): column 0 of knn_topk with the points as queries,
        bit for bit.  assign (optional, [N] int64 on the device) is the previous assignment, updated in place; moved counts the entries that
        changed (all N without a previous assignment)."""
        N, K = int(N), int(K)
        if assign is None:
            assign = torch.full((N,), -1, dtype=torch.int64, device=self.device)
        _check_dev(assign, "assign", self.device)
        if assign.dtype != torch.int64 or tuple(assign.shape) != (N,) or not assign.is_contiguous():
            raise ValueError("assign must be a contiguous int64 tensor of N entries")
        sims = torch.empty(N, dtype=_F32, device=self.device)
        moved = torch.zeros(1, dtype=torch.int32, device=self.device)
        p, n = self._compact_ws(N, K)
        self._ok(self.lib.tvc_index_assign_f32(self.ctx, self._stream(), _ptr(points_blob), N, _ptr(cent_blob), K, _ptr(assign), _ptr(sims), _ptr(moved), p, n),
                 "tvc_index_assign_f32")
        return assign, sims, moved

    def index_update(self, points_blob, N, assign, centroids):
        """centroids [768, K] fp32 (updated in place and returned): column k <- the mean of the raw vectors n of `points_blob` with
        assign[n] == k (fp64 sums in ascending n, rounded once); a cluster without members keeps its column, entries of assign outside
        [0, K) belong to no cluster -> (centroids, counts [K] int32)."""
        N = int(N)
        _check_dev(centroids, "centroids", self.device)
        if centroids.dtype != _F32 or centroids.dim() != 2 or centroids.shape[0] != spec.SSL_DIM or not centroids.is_contiguous():
            raise ValueError("centroids must be a contiguous fp32 [768, K] tensor")
        K = centroids.shape[1]
        assign = assign.to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(assign.shape) != (N,):
            raise ValueError("assign must have N entries")
        counts = torch.empty(K, dtype=torch.int32, device=self.device)
        p, n = self._compact_ws(N, K)
        self._ok(self.lib.tvc_index_update_f32(self.ctx, self._stream(), _ptr(points_blob), N, _ptr(assign), K, _ptr(centroids), _ptr(counts), p, n),
                 "tvc_index_update_f32")
        return centroids, counts

    def index_compact(self, points_blob, N, init_cols, iters):
        """k-means over the N raw vectors of `points_blob`: centroids start as the points init_cols [K] (int64), then `iters` rounds of
        (prepare, index_assign, index_update) in one call without a host synchronisation (tvc_index_compact_f32) ->
        (index [1, 768, K] fp32, its prepared blob, assign [N] int64, counts [K] int32, moved [iters] int32)."""
        N, iters = int(N), int(iters)
        init_cols = init_cols.to(device=self.device, dtype=torch.int64).contiguous()
        if init_cols.dim() != 1:
            raise ValueError("init_cols must be a 1-D list of point numbers")
        K = init_cols.numel()
        if not 4 <= K <= N:
            raise ValueError(f"index_compact: need 4 <= K <= N, got K = {K}, N = {N}")
        if iters < 1:
            raise ValueError("index_compact: iters >= 1")
        index = torch.empty(1, spec.SSL_DIM, K, dtype=_F32, device=self.device)
        blob = torch.empty(self.lib.tvc_knn_prepared_elems(K), dtype=_F32, device=self.device)
        assign = torch.empty(N, dtype=torch.int64, device=self.device)
        counts = torch.empty(K, dtype=torch.int32, device=self.device)
        moved = torch.empty(iters, dtype=torch.int32, device=self.device)
        p, n = self._compact_ws(N, K)
        self._ok(self.lib.tvc_index_compact_f32(self.ctx, self._stream(), _ptr(points_blob), N, _ptr(init_cols), K, iters, _ptr(index), _ptr(blob), _ptr(assign),
                                                _ptr(counts), _ptr(moved), p, n), "tvc_index_compact_f32")
        return index, self._owned(blob), assign, counts, moved

    def shift_frequency(self, f0, semitones):
        f0 = _prep(f0, "f0", self.device)
        out = torch.empty_like(f0)
        if f0.numel():
            self._ok(self.lib.tvc_shift_frequency_f32(self.ctx, self._stream(), _ptr(f0), _ptr(out), f0.numel(), float(semitones)), "tvc_shift_frequency_f32")
        return out

    def noise_angle_from_uniform(self, u):
        """u (fp32, contiguous, on the device) uniform in [0, 1) -> u * 2 * pi - pi in place: the reference's three tensor ops
        (decoder.py:78) as one launch with the same roundings."""
        _check_dev(u, "u", self.device)
        if u.dtype != _F32 or not u.is_contiguous():
            raise ValueError("u must be contiguous fp32")
        if u.numel():
            self._ok(self.lib.tvc_noise_angle_from_uniform_f32(self.ctx, self._stream(), _ptr(u), u.numel()), "tvc_noise_angle_from_uniform_f32")
        return u

    def _angle(self, noise_angle, B, T):
        if noise_angle is None and torch.cuda.is_current_stream_capturing():
            # inside a graph capture a kernel argument is baked in - one seed would replay for every launch of the graph -; torch's
            # generator is graph-safe (its offset advances per replay), so a captured call keeps the reference's torch.rand draw
            return self.noise_angle_from_uniform(torch.rand(B, spec.FFT_BIN, T, device=self.device)), 0
        if noise_angle is None:
            # the library draws the phases itself (tvc_* with noise_angle = NULL: a counter-based hash of (seed, row, bin, frame)).  Its
            # seed comes from THIS DEVICE's torch generator - the one the reference's torch.rand(device=...) draws from -: (seed, philox
            # offset) read on the host, the offset advanced as a draw would advance it.  No device launch, repeatable under
            # torch.manual_seed, untouched by CPU-side draws (module construction) in between.
            g = torch.cuda.default_generators[self.device.index if self.device.index is not None else torch.cuda.current_device()]
            off = g.get_offset()
            g.set_offset(off + 4)
            z = (g.initial_seed() * 0x9E3779B97F4A7C15 + off * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
            return None, z
        a = _prep(noise_angle, "noise_angle", self.device)
        if tuple(a.shape) != (B, spec.FFT_BIN, T):
            raise ValueError(f"noise_angle must be [{B}, {spec.FFT_BIN}, {T}], got {tuple(a.shape)}")
        return a, 0

    def decoder(self, content, f0, energy, noise_angle=None, stages=False):
        content = _prep(content, "content", self.device)
        f0 = _prep(f0, "f0", self.device)
        energy = _prep(energy, "energy", self.device)
        B, C, T = content.shape
        L = T * spec.HOP
        if C != spec.SSL_DIM or tuple(f0.shape) != (B, 1, T) or tuple(energy.shape) != (B, 1, L):
            raise ValueError(f"decoder shapes: content [B,768,T], f0 [B,1,T], energy [B,1,T*480]; got {tuple(content.shape)}, {tuple(f0.shape)}, {tuple(energy.shape)}")
        a, seed = self._angle(noise_angle, B, T)
        wave = torch.empty(B, L, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, L)
        if not stages:
            self._ok(self.lib.tvc_decoder_f32(self.ctx, self._stream(), _ptr(content), _ptr(f0), _ptr(energy), _ptr(a), seed, _ptr(wave), B, T, p, n), "tvc_decoder_f32")
            return wave
        amps = torch.empty(B, spec.NUM_HARMONICS + 1, T, dtype=_F32, device=self.device)
        kern = torch.empty(B, spec.FFT_BIN, T, dtype=_F32, device=self.device)
        source = torch.empty(B, 16, L, dtype=_F32, device=self.device)
        self._ok(self.lib.tvc_decoder_stages_f32(self.ctx, self._stream(), _ptr(content), _ptr(f0), _ptr(energy), _ptr(a), seed, _ptr(wave),
                                                 _ptr(amps), _ptr(kern), _ptr(source), B, T, p, n), "tvc_decoder_stages_f32")
        return wave, amps, kern, source

    def source_net(self, content, f0, energy):
        """SourceNet.forward (decoder.py:126-134) alone: (amps [B,15,T], kernel [B,961,T]) - no DSP, no FilterNet pass."""
        content = _prep(content, "content", self.device)
        f0 = _prep(f0, "f0", self.device)
        energy = _prep(energy, "energy", self.device)
        B, C, T = content.shape
        if C != spec.SSL_DIM or tuple(f0.shape) != (B, 1, T) or tuple(energy.shape) != (B, 1, T * spec.HOP):
            raise ValueError("source_net shapes: content [B,768,T], f0 [B,1,T], energy [B,1,T*480]")
        amps = torch.empty(B, spec.NUM_HARMONICS + 1, T, dtype=_F32, device=self.device)
        kern = torch.empty(B, spec.FFT_BIN, T, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, T * spec.HOP)
        self._ok(self.lib.tvc_decoder_stages_f32(self.ctx, self._stream(), _ptr(content), _ptr(f0), _ptr(energy), None, 0, None,
                                                 _ptr(amps), _ptr(kern), None, B, T, p, n), "tvc_decoder_stages_f32 (SourceNet)")
        return amps, kern

    def filter_net(self, content, f0, energy, source, blocks=False):
        """FilterNet.forward -> wave [B, L]; blocks=True also returns (skips[5], ups[4]): the Downsample / Upsample
        block outputs of decoder.py:227-232 (ups[4] is folded into the output conv, see tvc_filter_net_f32)."""
        content = _prep(content, "content", self.device)
        f0 = _prep(f0, "f0", self.device)
        energy = _prep(energy, "energy", self.device)
        source = _prep(source, "source", self.device)
        B, C, T = content.shape
        L = T * spec.HOP
        if C != spec.SSL_DIM or tuple(f0.shape) != (B, 1, T) or tuple(energy.shape) != (B, 1, L) or tuple(source.shape) != (B, 16, L):
            raise ValueError("filter_net shapes: content [B,768,T], f0 [B,1,T], energy [B,1,T*480], source [B,16,T*480]")
        wave = torch.empty(B, L, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, L)
        skips, ups, sk, up = None, None, None, None
        if blocks:
            ch, fac = spec.FILTER_CHANNELS, spec.FILTER_FACTORS
            dn = [L, L // 5, L // 20, L // 80, L // 240]
            skips = [torch.empty(B, ch[4 - i], dn[i], dtype=_F32, device=self.device) for i in range(5)]
            ups, l = [], T
            for i in range(4):
                l *= fac[i]
                ups.append(torch.empty(B, ch[i + 1], l, dtype=_F32, device=self.device))
            sk = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in skips])
            up = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ups])
        self._ok(self.lib.tvc_filter_net_f32(self.ctx, self._stream(), _ptr(content), _ptr(f0), _ptr(energy), _ptr(source), _ptr(wave),
                                             sk, up, B, T, p, n), "tvc_filter_net_f32")
        return (wave, skips, ups) if blocks else wave

    def dsp(self, f0, amps, kernel, noise_angle=None):
        f0 = _prep(f0, "f0", self.device)
        amps = _prep(amps, "amps", self.device)
        kernel = _prep(kernel, "kernel", self.device)
        B, _, T = f0.shape
        a, seed = self._angle(noise_angle, B, T)
        source = torch.empty(B, 16, T * spec.HOP, dtype=_F32, device=self.device)
        p, n = self._wsargs(B, T * spec.HOP)
        self._ok(self.lib.tvc_dsp_f32(self.ctx, self._stream(), _ptr(f0), _ptr(amps), _ptr(kernel), _ptr(a), seed, _ptr(source), B, T, p, n), "tvc_dsp_f32")
        return source

    def stream_push(self, buf, blocks):
        """buf [S, n] <- (buf[:, m:], blocks [S, m]) in place, one launch for any buffer length n >= m (stream.py:69-70's roll + slice
        assignment)."""
        _check_dev(buf, "buf", self.device)
        blocks = _prep(blocks, "blocks", self.device)
        S, n = buf.shape
        if blocks.shape[0] != S or not buf.is_contiguous() or buf.dtype != _F32:
            raise ValueError("stream_push: buf [S, n] contiguous fp32, blocks [S, m] with m <= n (n of any length)")
        self._ok(self.lib.tvc_stream_push_f32(self.ctx, self._stream(), _ptr(buf), _ptr(blocks), S, n, blocks.shape[1]), "tvc_stream_push_f32")
        return buf

    def sola(self, y, sola_buf, fade_in, block, use_phase_vocoder=False, want_shift=False, crossfade=None, search=None, delay=None):
        """y [S, Ly]; sola_buf [S, crossfade] updated in place; fade_in [crossfade]; returns out [S, block] (and shifts).  The geometry
        (tvc_sola_geom_f32; None = the reference's 1920 / 1920 / 3840) is checked by the library, the two tensors against it here: the
        kernels read `crossfade` floats of each."""
        y = _prep(y, "y", self.device)
        _check_dev(sola_buf, "sola_buffer", self.device)
        fade_in = _prep(fade_in, "fade_in_window", self.device)
        if not sola_buf.is_contiguous() or sola_buf.dtype != _F32:
            raise ValueError("sola_buffer must be contiguous fp32")
        default = crossfade is None and search is None and delay is None
        cross, search, delay = (d if x is None else x for x, d in ((crossfade, SOLA_CROSS), (search, SOLA_SEARCH), (delay, SOLA_DELAY)))
        cross, search, delay = (integer(x, "sola", name) for x, name in ((cross, "crossfade"), (search, "search"), (delay, "delay")))      # as sola_geometry
        S, Ly = y.shape
        if tuple(sola_buf.shape) != (S, cross) or fade_in.numel() != cross:
            raise ValueError(f"sola: crossfade = {cross} takes sola_buffer [{S}, {cross}] and a fade_in_window of {cross} entries, got "
                             f"{tuple(sola_buf.shape)} and {fade_in.numel()}")
        out = torch.empty(S, max(int(block), 0), dtype=_F32, device=self.device)
        shift = torch.empty(S, dtype=torch.int32, device=self.device) if want_shift else None
        if default:      # tvc_sola_f32 is the (1920, 1920, 3840) call of the same implementation and keeps its own error text
            self._ok(self.lib.tvc_sola_f32(self.ctx, self._stream(), _ptr(y), _ptr(sola_buf), _ptr(fade_in), _ptr(out), _ptr(shift), S, Ly, int(block),
                                           int(bool(use_phase_vocoder))), "tvc_sola_f32")
        else:
            self._ok(self.lib.tvc_sola_geom_f32(self.ctx, self._stream(), _ptr(y), _ptr(sola_buf), _ptr(fade_in), _ptr(out), _ptr(shift), S, Ly, int(block),
                                                cross, search, delay, int(bool(use_phase_vocoder))), "tvc_sola_geom_f32")
        return (out, shift) if want_shift else out

    def stream_gate(self, x, y, shift, gate, base, out=None):
        """The noise gate behind the tail (tvc_stream_gate_f32): x [S, n] the streams' input windows, y [S, block] the emitted blocks,
        shift [S] int32 the tail's lags (None = 0), `gate` a module.infer.StreamGate (thresholds and state on the device, advanced in place),
        base + shift[s] the index in x[s] of the input sample y[s, 0] was converted from.  Returns the gated blocks: a new tensor, or `out`
        (which may be y)."""
        for t, name in ((x, "x"), (y, "y")):
            _check_dev(t, name, self.device)
            if t.dim() != 2 or t.dtype != _F32 or not t.is_contiguous():
                raise ValueError(f"stream_gate: {name} must be contiguous fp32 [S, n], got {t.dtype} {tuple(t.shape)}")
        S, n = x.shape
        if tuple(y.shape) != (S, gate.block_size) or gate.n_streams != S:
            raise ValueError(f"stream_gate: a gate for {gate.n_streams} streams of {gate.block_size}-sample blocks, x is {tuple(x.shape)} and y {tuple(y.shape)}")
        if shift is not None:
            _check_dev(shift, "shift", self.device)
            if shift.dtype != torch.int32 or tuple(shift.shape) != (S,) or not shift.is_contiguous():
                raise ValueError(f"stream_gate: shift must be contiguous int32 [{S}], got {shift.dtype} {tuple(shift.shape)}")
        if isinstance(base, bool) or not isinstance(base, numbers.Integral):
            raise ValueError(f"stream_gate: base must be an integer, got {base!r}")
        state = checked(gate, GATE_STATE, S, self.device, "stream_gate: gate.")
        if out is None:
            out = torch.empty_like(y)
        else:
            _check_dev(out, "out", self.device)
            if out.dtype != _F32 or out.shape != y.shape or not out.is_contiguous():
                raise ValueError(f"stream_gate: out must be contiguous fp32 {tuple(y.shape)}, got {out.dtype} {tuple(out.shape)}")
        sub, look, hold, attack, release, hysteresis_db, range_db = gate.params()[2:]
        self._ok(self.lib.tvc_stream_gate_f32(self.ctx, self._stream(), _ptr(x), n, int(base), _ptr(shift), _ptr(y), _ptr(out), S, gate.block_size, sub, look,
                                              hold, attack, release, hysteresis_db, range_db, *map(_ptr, state)), "tvc_stream_gate_f32")
        return out

    def loudness_match(self, x, y, share, lengths=None, settings=None, out=None, want_gains=False):
        """The loudness envelope match (tvc_loudness_match_f32; its definition is in tinyvc_hip.h): x [B, L] the input on the output's time
        axis, y [B, L] the converted waves, share [B] fp32 on the device (read when the kernel runs), `lengths` a ragged batch's row lengths
        (a sequence on the host: they travel as kernel arguments, so the call stays asynchronous and capturable), `settings` anything with
        sub_frame, smooth, floor_db, boost_db and cut_db (a feature_retrieval.LoudnessMatch; None: the defaults).  Returns the matched waves
        - a new tensor, or `out`, which may be y (one workgroup per row then: see loudness_in_place) - and with want_gains the gain at every
        sub-frame edge, [B, L / sub_frame + 1]."""
        for t, name in ((x, "x"), (y, "y")):
            _check_dev(t, name, self.device)
            if t.dim() != 2 or t.dtype != _F32 or not t.is_contiguous():
                raise ValueError(f"loudness_match: {name} must be contiguous fp32 [B, L], got {t.dtype} {tuple(t.shape)}")
        B, L = y.shape
        if x.shape != y.shape:
            raise ValueError(f"loudness_match: x {tuple(x.shape)} and y {tuple(y.shape)} must have one shape")
        _check_dev(share, "share", self.device)
        if share.dtype != _F32 or tuple(share.shape) != (B,) or not share.is_contiguous():
            raise ValueError(f"loudness_match: share must be contiguous fp32 [{B}], got {share.dtype} {tuple(share.shape)}")
        sub, smooth, floor_db, boost_db, cut_db = ((240, 2, -60.0, 12.0, 40.0) if settings is None else
                                                   (settings.sub_frame, settings.smooth, settings.floor_db, settings.boost_db, settings.cut_db))
        nsub = loudness_geometry(L, sub, smooth, lib=self.lib)[0]
        floor_db, boost_db, cut_db = loudness_levels(floor_db, boost_db, cut_db, "loudness_match")
        lens = None
        if lengths is not None:
            vals = lengths.tolist() if isinstance(lengths, torch.Tensor) and lengths.device.type == "cpu" else lengths
            if isinstance(vals, torch.Tensor) or len(vals) != B or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) for n in vals):
                raise ValueError(f"loudness_match: lengths: a host sequence of one integer per row ({B}), got {lengths!r}")
            if min(vals) < 0 or max(vals) > L or any(n % sub for n in vals):
                raise ValueError(f"loudness_match: lengths: one entry per row, each a whole number of {sub}-sample sub-frames in 0 .. {L}")
            lens = (ctypes.c_int64 * B)(*[int(n) for n in vals])
        if out is None:
            out = torch.empty_like(y)
        else:
            _check_dev(out, "out", self.device)
            if out.dtype != _F32 or out.shape != y.shape or not out.is_contiguous():
                raise ValueError(f"loudness_match: out must be contiguous fp32 {tuple(y.shape)}, got {out.dtype} {tuple(out.shape)}")
        gains = torch.empty(B, nsub + 1, dtype=_F32, device=self.device) if want_gains else None
        self._ok(self.lib.tvc_loudness_match_f32(self.ctx, self._stream(), _ptr(x), _ptr(y), _ptr(out), B, L, lens, _ptr(share), sub, smooth, floor_db,
                                                 boost_db, cut_db, _ptr(gains)), "tvc_loudness_match_f32")
        return (out, gains) if want_gains else out

    def stream_loudness(self, x, y, shift, stage, base, out=None, want_gains=False):
        """The loudness envelope match behind the tail (tvc_stream_loudness_f32), with stream_gate's addressing: x [S, n] the streams' input
        windows, y [S, block] the emitted blocks, shift [S] int32 the tail's lags (None = 0), base + shift[s] the index in x[s] of the input
        sample y[s, 0] was converted from; `stage` a module.infer.StreamLoudness (share and state on the device, advanced in place).  Returns
        the matched blocks - a new tensor, or `out` (which may be y) - and with want_gains the block's edge gains [S, block / sub_frame + 1]."""
        for t, name in ((x, "x"), (y, "y")):
            _check_dev(t, name, self.device)
            if t.dim() != 2 or t.dtype != _F32 or not t.is_contiguous():
                raise ValueError(f"stream_loudness: {name} must be contiguous fp32 [S, n], got {t.dtype} {tuple(t.shape)}")
        S, n = x.shape
        if tuple(y.shape) != (S, stage.block_size) or stage.n_streams != S:
            raise ValueError(f"stream_loudness: a stage for {stage.n_streams} streams of {stage.block_size}-sample blocks, x is {tuple(x.shape)} and y "
                             f"{tuple(y.shape)}")
        if shift is not None:
            _check_dev(shift, "shift", self.device)
            if shift.dtype != torch.int32 or tuple(shift.shape) != (S,) or not shift.is_contiguous():
                raise ValueError(f"stream_loudness: shift must be contiguous int32 [{S}], got {shift.dtype} {tuple(shift.shape)}")
        if isinstance(base, bool) or not isinstance(base, numbers.Integral):
            raise ValueError(f"stream_loudness: base must be an integer, got {base!r}")
        state = checked(stage, LOUDNESS_STATE, S, self.device, "stream_loudness: loudness.")
        if out is None:
            out = torch.empty_like(y)
        else:
            _check_dev(out, "out", self.device)
            if out.dtype != _F32 or out.shape != y.shape or not out.is_contiguous():
                raise ValueError(f"stream_loudness: out must be contiguous fp32 {tuple(y.shape)}, got {out.dtype} {tuple(out.shape)}")
        sub, smooth, floor_db, boost_db, cut_db = stage.params()[2:]
        gains = torch.empty(S, stage.block_size // sub + 1, dtype=_F32, device=self.device) if want_gains else None
        self._ok(self.lib.tvc_stream_loudness_f32(self.ctx, self._stream(), _ptr(x), n, int(base), _ptr(shift), _ptr(y), _ptr(out), S, stage.block_size, sub,
                                                  smooth, floor_db, boost_db, cut_db, *map(_ptr, state), _ptr(gains)), "tvc_stream_loudness_f32")
        return (out, gains) if want_gains else out

    def limit(self, y, ceiling, lengths=None, settings=None, want_gains=False):
        """The look-ahead peak limiter (tvc_limit_f32; its definition is in tinyvc_hip.h): y [B, L] the waves, ceiling [B] fp32 on the device,
        linear amplitudes read when the kernel runs (NaN, <= 0 and inf: off), `lengths` a ragged batch's row lengths (a sequence on the
        host: they travel as kernel arguments, so the call stays asynchronous and capturable), `settings` anything with sub_frame, release
        (sub-frames) and drive_db (a feature_retrieval.Limiter; None: the defaults).  Returns the limited waves, always a new tensor - no
        sample of a row's own length lies above its ceiling -, and with want_gains the gain at every sub-frame edge, [B, L / sub_frame + 1]."""
        _check_dev(y, "y", self.device)
        if y.dim() != 2 or y.dtype != _F32 or not y.is_contiguous():
            raise ValueError(f"limit: y must be contiguous fp32 [B, L], got {y.dtype} {tuple(y.shape)}")
        B, L = y.shape
        _check_dev(ceiling, "ceiling", self.device)
        if ceiling.dtype != _F32 or tuple(ceiling.shape) != (B,) or not ceiling.is_contiguous():
            raise ValueError(f"limit: ceiling must be contiguous fp32 [{B}], got {ceiling.dtype} {tuple(ceiling.shape)}")
        sub, release, drive_db = (24, 100, 0.0) if settings is None else (settings.sub_frame, settings.release, settings.drive_db)
        nsub = limiter_geometry(L, sub, release, lib=self.lib)[0]
        drive_db = limiter_drive(drive_db, "limit")
        lens = None
        if lengths is not None:
            vals = lengths.tolist() if isinstance(lengths, torch.Tensor) and lengths.device.type == "cpu" else lengths
            if isinstance(vals, torch.Tensor) or len(vals) != B or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) for n in vals):
                raise ValueError(f"limit: lengths: a host sequence of one integer per row ({B}), got {lengths!r}")
            lens = (ctypes.c_int64 * B)(*[int(n) for n in vals])      # (the kernel clamps them to 0 .. L and to whole sub-frames)
        out = torch.empty_like(y)
        gains = torch.empty(B, nsub + 1, dtype=_F32, device=self.device) if want_gains else None
        self._ok(self.lib.tvc_limit_f32(self.ctx, self._stream(), _ptr(y), _ptr(out), B, L, lens, _ptr(ceiling), sub, release, drive_db, _ptr(gains)),
                 "tvc_limit_f32")
        return (out, gains) if want_gains else out

    def stream_limit(self, y, stage, want_gains=False):
        """The peak limiter at the end of a stream's block (tvc_stream_limit_f32): y [S, block] the blocks, `stage` a module.infer.StreamLimiter
        (ceiling and state on the device, advanced in place).  Returns the limited blocks, a new tensor `stage.sub_frame` samples behind y -
        the sub-frame held back is the stage's look-ahead -, and with want_gains the block's edge gains [S, block / sub_frame + 1]."""
        _check_dev(y, "y", self.device)
        if y.dim() != 2 or y.dtype != _F32 or not y.is_contiguous():
            raise ValueError(f"stream_limit: y must be contiguous fp32 [S, block], got {y.dtype} {tuple(y.shape)}")
        S = y.shape[0]
        if tuple(y.shape) != (stage.n_streams, stage.block_size):
            raise ValueError(f"stream_limit: a stage for {stage.n_streams} streams of {stage.block_size}-sample blocks, y is {tuple(y.shape)}")
        state = checked(stage, LIMITER_STATE, S, self.device, "stream_limit: limiter.")
        sub, release, drive_db = stage.params()[2:]
        out = torch.empty_like(y)
        gains = torch.empty(S, stage.block_size // sub + 1, dtype=_F32, device=self.device) if want_gains else None
        self._ok(self.lib.tvc_stream_limit_f32(self.ctx, self._stream(), _ptr(y), _ptr(out), S, stage.block_size, sub, release, drive_db, *map(_ptr, state),
                                               _ptr(gains)), "tvc_stream_limit_f32")
        return (out, gains) if want_gains else out

    def stream_denoise(self, blocks, denoise, out=None):
        """The spectral suppressor in front of the window (tvc_stream_denoise_f32): blocks [S, block] the streams' new 24 kHz samples,
        `denoise` a module.infer.StreamDenoise (reduction and state on the device, advanced in place).  Returns the suppressed blocks,
        delayed by denoise.delay_size samples: a new tensor, or `out` (which may be blocks)."""
        _check_dev(blocks, "blocks", self.device)
        if blocks.dim() != 2 or blocks.dtype != _F32 or not blocks.is_contiguous():
            raise ValueError(f"stream_denoise: blocks must be contiguous fp32 [S, block], got {blocks.dtype} {tuple(blocks.shape)}")
        S = blocks.shape[0]
        if tuple(blocks.shape) != (denoise.n_streams, denoise.block_size):
            raise ValueError(f"stream_denoise: a suppressor for {denoise.n_streams} streams of {denoise.block_size}-sample blocks, blocks is {tuple(blocks.shape)}")
        state = checked(denoise, DENOISE_STATE, S, self.device, "stream_denoise: denoise.")
        if out is None:
            out = torch.empty_like(blocks)
        else:
            _check_dev(out, "out", self.device)
            if out.dtype != _F32 or out.shape != blocks.shape or not out.is_contiguous():
                raise ValueError(f"stream_denoise: out must be contiguous fp32 {tuple(blocks.shape)}, got {out.dtype} {tuple(out.shape)}")
        hop, a_s, a_n, clamp, beta, warm = denoise.params()[2:]
        self._ok(self.lib.tvc_stream_denoise_f32(self.ctx, self._stream(), _ptr(blocks), _ptr(out), S, denoise.block_size, hop, a_s, a_n, clamp, beta, warm,
                                                 *map(_ptr, state)), "tvc_stream_denoise_f32")
        return out


# ---------------------------------------------------------------------- shared weightless engines
_default = {}
_lock = threading.Lock()


def default_engine(device):
    """Engine without checkpoint weights, for the free functions of module.utils / match_features."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.TinyVCError(f"tinyvc_amd runs on an AMD GPU only; got a tensor on {device}")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _lock:
        if idx not in _default:
            _default[idx] = Engine(torch.device("cuda", idx))
        return _default[idx]
