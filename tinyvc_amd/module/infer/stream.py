"""Real-time wrapper: rolling input buffer, full convert per block, SOLA alignment and cross-fade
(reference module/infer/stream.py:30-96).  `StreamInfer` is the reference's single-stream class;
`BatchedStreamInfer` runs S independent streams through one batched convert + one SOLA launch with
the lag arg-max kept on the device.  The tail's geometry (extension: the reference hard-codes it, stream.py:48-50) is a constructor
argument - crossfade_size, sola_search_size, last_delay_size -: a block's first sample leaves crossfade + search + delay - shift samples
after the first sample of the newest input block came in (shift in [0, search], chosen per block), so the three sizes are the latency a
listener hears beyond the block itself; look-ahead (last_delay_size) is the right context the converter sees behind the emitted block.  `StreamDoor` (extension) puts a stateful resampler, fused with the int16 conversions and gain, on both
sides of the block: clients send and receive int16 at their own rates.  `StreamGate` (extension) is a per-stream noise gate on the device,
one launch behind SOLA: it follows the input window's power under the emitted block and looks ahead in what the window already holds.
`StreamDenoise` (extension) is a per-stream spectral suppressor on the device, one launch in front of the window: noise under speech is
turned down before the converter, the pitch tracker and the gate see it.  `StreamLoudness` (extension) makes every emitted block follow the
loudness envelope of the input it was converted from, one launch behind SOLA and in front of the gate.  `StreamLimiter` (extension) is a
look-ahead peak limiter, the last launch in front of the door's output side: no sample leaves above a stream's ceiling."""
import math

import numpy as np
import torch

from ...engine import (SOLA_CROSS, SOLA_DELAY, SOLA_SEARCH, loudness_geometry, loudness_levels, pitch_shifts, sola_geometry, stream_denoise_geometry,
                       stream_gate_geometry, stream_resample_geometry)
from ...stream_state import CARRY_STATE, SNAP_STATE, DENOISE_STATE, DOOR_STATE, GATE_STATE, LIMITER_STATE, LOUDNESS_STATE, TRACK_STATE, addresses, allocate, reset
from ..tinyvc.feature_retrieval import (PitchCarry, PitchTrack, SnapCarry, alpha_rows, continuity_rows, resolve_continuity, match_k_rows, match_width_rows, resolve_match_k, resolve_match_width, check_f0_carry, check_stream_tune, gpu_device, limit_ceiling, limiter_settings, protect_rows, resolve_alpha,
                                        resolve_auto_pitch, resolve_f0_estimation, resolve_protect, target_form)
from .generator import Generator


def _fade_windows(crossfade_size, device):
    # stream.py:61-62, computed on the host exactly as the reference does, then uploaded.  The window is the FIRST crossfade_size entries
    # of the reference's expression: with a floating-point step arange(0, 1, 1 / n) has n + 1 entries for some n (196, 392, 412, ...)
    fade_in = torch.sin(np.pi * torch.arange(0, 1, 1 / crossfade_size)[:crossfade_size] / 2) ** 2
    assert fade_in.numel() == crossfade_size
    return fade_in.to(device), (1 - fade_in).to(device)


MIN_INPUT = 960      # the front end reflect-pads a window by 960 samples on either side: it takes windows longer than that
FRAME = 480


def check_window(block_size, extra_size, crossfade_size, sola_search_size, last_delay_size, auto_pitch):
    """The geometry of a stream against everything that can be said on the host (ValueError) -> (input_size, pad).  convert zero-pads a
    window at its END to whole 480-sample frames and returns the padded length, and the tail counts from the end of what convert returns: a
    window of input_size samples that is not whole frames puts pad = -input_size % 480 samples of converted padding behind the signal, so the
    tail's look-ahead over the SIGNAL is last_delay_size - pad.  It must not be negative: the emitted block and the next SOLA buffer would
    be cut partly from the conversion of the padding."""
    sola_geometry(block_size, crossfade_size, sola_search_size, last_delay_size)      # ValueError with the library's reason
    input_size = max(block_size + crossfade_size + sola_search_size + 2 * last_delay_size, block_size + extra_size)
    if input_size <= MIN_INPUT:
        raise ValueError(f"the stream's window of {input_size} samples (the larger of block + crossfade + search + 2 * delay and block + extra_size) "
                         f"is too short for the front end, which reflect-pads {MIN_INPUT} samples on either side: raise extra_size to more than "
                         f"{MIN_INPUT - block_size}")
    pad = -input_size % FRAME
    if pad > last_delay_size:
        whole = (input_size + pad) - block_size
        raise ValueError(f"the stream's window of {input_size} samples is converted as {input_size + pad} (whole {FRAME}-sample frames, zeros at the end): "
                         f"{pad} samples of padding behind a look-ahead of last_delay_size = {last_delay_size} would put converted padding into the "
                         f"emitted block; extra_size = {whole} makes the window whole frames")
    if auto_pitch and last_delay_size % FRAME:
        raise ValueError(f"auto_pitch: last_delay_size = {last_delay_size} is not a whole number of 480-sample frames (the tracker's new frames "
                         f"end that far before the end of the window)")
    return input_size, pad


MODEL_RATE = 24000


class StreamDoor:
    """The two resamplers of a set of streams that advance in lock step (tvc_stream_resample): clients send int16 at `in_rate` and receive
    int16 at `out_rate` (default: in_rate); the model runs `block_size` samples at 24 kHz in between.
      chunk_in, chunk_out      the client-side block lengths: block_size * in_rate / 24000 and block_size * out_rate / 24000
      in_state [S, hist_in]    each stream's filter history on the way in (client samples after the int16 conversion and input_gain)
      out_state [S, hist_out]  and on the way out (24 kHz samples), fp32 on the device; zeros = the start of a stream
      latency_seconds          delay_in / 24000 + delay_out / out_rate: what the two filters' look-ahead adds
    A stream's blocks are, bit for bit, what the offline resampler gives for the whole signal with G * orig zeros in front (see
    tinyvc_hip.h).  `input_gain` / `output_gain` in dB, applied with the int16 conversions.  Every argument is checked before anything is
    allocated (ValueError): a block_size either rate cannot serve in whole groups is refused with the nearest sizes that work."""

    def __init__(self, n_streams, in_rate, out_rate=None, block_size=1920, input_gain=0.0, output_gain=0.0, device=None):
        out_rate = in_rate if out_rate is None else out_rate
        for x, name in ((n_streams, "n_streams"), (in_rate, "in_rate"), (out_rate, "out_rate"), (block_size, "block_size")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"StreamDoor: {name} must be an integer >= 1, got {x!r}")
        for x, name in ((input_gain, "input_gain"), (output_gain, "output_gain")):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError(f"StreamDoor: {name} must be a finite number of dB, got {x!r}")
        # the 24 kHz side of each rate pair comes in groups of 24000 / gcd samples: the block must be whole groups of both
        step = math.lcm(MODEL_RATE // math.gcd(in_rate, MODEL_RATE), MODEL_RATE // math.gcd(out_rate, MODEL_RATE))
        if block_size % step:
            near = [n for n in (block_size // step * step, (block_size // step + 1) * step) if n > 0]
            raise ValueError(f"StreamDoor: block_size = {block_size} at 24000 Hz is not a whole number of resampling groups for {in_rate} Hz in / "
                             f"{out_rate} Hz out (multiples of {step}); the nearest sizes that work: {' or '.join(str(n) for n in near)}")
        self.n_streams, self.in_rate, self.out_rate, self.block_size = n_streams, in_rate, out_rate, block_size
        self.input_gain, self.output_gain = float(input_gain), float(output_gain)
        self.chunk_in = block_size * in_rate // MODEL_RATE
        self.chunk_out = block_size * out_rate // MODEL_RATE
        n24, self.hist_in, self.delay_in = stream_resample_geometry(in_rate, MODEL_RATE, self.chunk_in)
        nout, self.hist_out, self.delay_out = stream_resample_geometry(MODEL_RATE, out_rate, block_size)
        assert (n24, nout) == (block_size, self.chunk_out)
        self.latency_seconds = self.delay_in / MODEL_RATE + self.delay_out / out_rate
        self.device = gpu_device(device, "StreamDoor: the state lives on the GPU, where the door's kernel runs")
        allocate(self, DOOR_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in"""
        return (self.in_rate, self.out_rate, self.block_size, self.input_gain, self.output_gain)

    def prepare(self, engine):
        """build `engine`'s filter tables for both rate pairs now: their first use allocates, which a graph capture cannot record"""
        engine.stream_resample_prepare(self.in_rate, MODEL_RATE)
        engine.stream_resample_prepare(MODEL_RATE, self.out_rate)

    def reset(self, streams=None):
        """Forget the filter history of every stream, or of the listed ones: in-place ops on the state tensors, so it works between replays
        of a captured graph (which reads them when it runs)."""
        reset(self, DOOR_STATE, streams)

    def push(self, engine, pcm):
        """client int16 [S, chunk_in] -> fp32 [S, block_size] at 24 kHz (input_gain applied), advancing in_state"""
        return engine.stream_resample(pcm, self.in_state, self.in_rate, MODEL_RATE, self.input_gain)

    def pull(self, engine, y):
        """fp32 [S, block_size] at 24 kHz -> client int16 [S, chunk_out] (output_gain applied), advancing out_state"""
        return engine.stream_resample(y, self.out_state, MODEL_RATE, self.out_rate, self.output_gain, out_pcm16=True)


def check_gate_lookahead(lookahead_size, crossfade_size, last_delay_size, pad_size):
    """The gate's look-ahead against the window (ValueError): behind the input samples of an emitted block the window holds crossfade + search +
    delay - shift more, of which the last pad_size belong to a frame the converter padded; at the largest lag that leaves crossfade_size +
    last_delay_size - pad_size input samples the gate may look at without running past the window's end."""
    room = crossfade_size + last_delay_size - pad_size
    if lookahead_size > room:
        raise ValueError(f"gate: lookahead_size = {lookahead_size} is more than the {room} input samples the window holds behind an emitted block "
                         f"(crossfade_size {crossfade_size} + last_delay_size {last_delay_size} - pad_size {pad_size})")
    return room


def _db_rows(x, n_streams, refusal):
    """a live per-stream parameter in dB as given - a number, one per stream, or a 1-D tensor - -> n_streams floats; ValueError(refusal) for
    anything else, NaN included"""
    vals = [x] if isinstance(x, (int, float)) and not isinstance(x, bool) else x
    if isinstance(vals, torch.Tensor):
        vals = vals.detach().cpu().tolist() if vals.dim() == 1 else None
    if not isinstance(vals, (list, tuple)) or len(vals) not in (1, n_streams) or not all(
            isinstance(t, (int, float)) and not isinstance(t, bool) and not math.isnan(t) for t in vals):
        raise ValueError(refusal)
    return [float(t) for t in vals] * (n_streams // len(vals))


class StreamGate:
    """The noise gate of a set of streams that advance in lock step (tvc_stream_gate_f32; its definition is in tinyvc_hip.h): behind SOLA,
    every emitted block is multiplied by a gain that follows the power of the INPUT samples it was converted from, sub-frame by sub-frame,
    and of `lookahead_size` samples of input behind them, which the rolling window already holds - so the gate opens ahead of an onset at no
    added latency.  It never feeds back: the SOLA buffer and the window stay ungated, and closed streams are still converted.
      threshold_db [S]   fp32 on the device, read when a block runs: a sub-frame at or above it (mean power, dB re full scale) opens the gate;
                         `gate.threshold_db.fill_(...)` / `copy_(...)` moves it between blocks; -inf = always open, the ungated stream bit for bit
      hysteresis_db      the gate stays open down to threshold - hysteresis
      hold_size, attack_size, release_size, lookahead_size
                         24 kHz samples, whole sub-frames: how long an open gate outlasts the last loud sub-frame, how long the gain takes
                         from 0 to 1 and from 1 to 0 (at least one sub-frame each), how far the gate looks ahead
      range_db           the gain of a closed gate (<= 0; -inf, the default: silence)
      gain [S] fp32, open [S] int32, hold [S] int32      the state the next block starts from; level_db [S]: the last block's input level
    The defaults are guesses: nobody has listened to them yet.  Every argument is checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, block_size, threshold_db=-50.0, hysteresis_db=6.0, hold_size=4800, attack_size=240, release_size=2400,
                 lookahead_size=480, sub_frame=240, range_db=-math.inf, device=None):
        for x, name in ((n_streams, "n_streams"), (block_size, "block_size"), (sub_frame, "sub_frame")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"StreamGate: {name} must be an integer >= 1, got {x!r}")
        for x, name, least in ((hold_size, "hold_size", 0), (attack_size, "attack_size", 1), (release_size, "release_size", 1),
                               (lookahead_size, "lookahead_size", 0)):
            if isinstance(x, bool) or not isinstance(x, int) or x < 0 or x % sub_frame or x // sub_frame < least:
                raise ValueError(f"StreamGate: {name} must be a whole number of {sub_frame}-sample sub-frames, at least {least}; got {x!r}")
        thr = _db_rows(threshold_db, n_streams,
                       f"StreamGate: threshold_db must be a number of dB (-inf: always open) or one per stream ({n_streams}), got {threshold_db!r}")
        if isinstance(hysteresis_db, bool) or not isinstance(hysteresis_db, (int, float)) or not math.isfinite(hysteresis_db) or hysteresis_db < 0:
            raise ValueError(f"StreamGate: hysteresis_db must be a finite number of dB >= 0, got {hysteresis_db!r}")
        if isinstance(range_db, bool) or not isinstance(range_db, (int, float)) or not range_db <= 0:
            raise ValueError(f"StreamGate: range_db must be a number of dB <= 0 (-inf: a closed gate is silent), got {range_db!r}")
        self.look, self.hold_count, self.attack, self.release = (v // sub_frame for v in (lookahead_size, hold_size, attack_size, release_size))
        try:
            stream_gate_geometry(block_size, sub_frame, self.look, self.hold_count, self.attack, self.release)
        except ValueError as e:
            raise ValueError(f"StreamGate: {e}") from None
        self.n_streams, self.block_size, self.sub_frame = n_streams, block_size, sub_frame
        self.hold_size, self.attack_size, self.release_size, self.lookahead_size = hold_size, attack_size, release_size, lookahead_size
        self.hysteresis_db, self.range_db = float(hysteresis_db), float(range_db)
        self.device = gpu_device(device, "StreamGate: the thresholds and the state live on the GPU, where the gate's kernel runs")
        self.threshold_db = torch.tensor(thr, dtype=torch.float32, device=self.device)
        allocate(self, GATE_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in: (n_streams, block_size, sub_frame, look, hold, attack, release - counts of sub-frames -,
        hysteresis_db, range_db)"""
        return (self.n_streams, self.block_size, self.sub_frame, self.look, self.hold_count, self.attack, self.release, self.hysteresis_db, self.range_db)

    def reset(self, streams=None):
        """Put every stream, or the listed ones, back at the start: open, no hold left, gain 1 (a silent start then closes over release_size).
        In-place ops on the state tensors, so it works between replays of a captured graph, which reads them when it runs."""
        reset(self, GATE_STATE, streams)


def _f32(x):
    with np.errstate(over="ignore"):      # too large for fp32 is inf, which the callers refuse
        return float(np.float32(x))


def denoise_constants(hop, strength, smooth_ms, adapt_s, clamp, warmup_ms):
    """The suppressor's baked constants from its settings (ValueError) -> (a_s, a_n, clamp, beta, warm): the two recurrence coefficients
    a = exp(-hop / (24000 * time constant)), computed in double and rounded to fp32 once (0 for a time constant of 0), clamp and beta =
    strength as fp32 values, and the warm-up in frames, round(warmup * 24000 / hop).  This is the one place they are computed."""
    for x, name, least in ((strength, "strength", 0.0), (smooth_ms, "smooth_ms", 0.0), (adapt_s, "adapt_s", 0.0), (clamp, "clamp", 1.0),
                           (warmup_ms, "warmup_ms", 0.0)):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < least:
            raise ValueError(f"StreamDenoise: {name} must be a finite number >= {least:g}, got {x!r}")
    a_s = _f32(math.exp(-hop / (MODEL_RATE * smooth_ms * 1e-3))) if smooth_ms > 0 else 0.0
    a_n = _f32(math.exp(-hop / (MODEL_RATE * adapt_s))) if adapt_s > 0 else 0.0
    if a_s >= 1.0 or a_n >= 1.0:
        raise ValueError(f"StreamDenoise: smooth_ms = {smooth_ms!r} or adapt_s = {adapt_s!r} is so long that its fp32 coefficient is 1: nothing would move")
    beta, clamp = _f32(strength), _f32(clamp)
    if not math.isfinite(beta) or not math.isfinite(clamp):
        raise ValueError(f"StreamDenoise: strength = {strength!r} or clamp = {clamp!r} is not a finite fp32 number")
    warm = int(round(warmup_ms * 1e-3 * MODEL_RATE / hop))
    if warm >= 2 ** 30:
        raise ValueError(f"StreamDenoise: warmup_ms = {warmup_ms!r} is more than 2^30 frames")
    return a_s, a_n, clamp, beta, warm


class StreamDenoise:
    """The spectral suppressor of a set of streams that advance in lock step (tvc_stream_denoise_f32; its definition is in tinyvc_hip.h): in
    front of the rolling window every 24 kHz block goes through a short-time spectral gain - 640-sample frames under a square-root Hann
    window at a hop of `hop` samples, a noise estimate per bin, G = max(floor, 1 - strength * noise / smoothed power), overlap-add - so the
    window, and with it the converter, the pitch tracker and the gate, see the suppressed signal `delay_size` = 640 - hop samples late.
      reduction_db [S]   fp32 on the device, read when a block runs: the most a bin is turned down by (floor = 10^(-reduction_db / 20); 0 or
                         less: the delayed input); `denoise.reduction_db.fill_(...)` / `copy_(...)` moves it between blocks
      hop                160 or 320 samples: 20 ms or 13.3 ms of delay, four or two frames over every sample
      strength           the over-subtraction factor beta
      smooth_ms          time constant of the smoothed power the gain is computed from
      adapt_s            time constant of the noise estimate once the warm-up is over; it follows a bin up by at most `clamp` times itself
                         per frame, so speech moves it slowly and a lasting change of the noise is followed
      warmup_ms          the first frames of a stream that are not all zeros are taken for noise: a running mean over that long
      hist, ola [S, delay_size], smooth, noise [S, 321], frames [S] int32      the state the next block starts from
      noise_db [S]       the noise estimate after the last block, dB re full scale per sample: a guide for a gate's threshold
    The defaults are guesses: nobody has listened to them yet.  Every argument is checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, block_size, reduction_db=12.0, hop=160, strength=2.0, smooth_ms=40.0, adapt_s=1.0, clamp=2.0, warmup_ms=200.0,
                 device=None):
        for x, name in ((n_streams, "n_streams"), (block_size, "block_size"), (hop, "hop")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"StreamDenoise: {name} must be an integer >= 1, got {x!r}")
        red = _db_rows(reduction_db, n_streams,
                       f"StreamDenoise: reduction_db must be a number of dB (0: no suppression) or one per stream ({n_streams}), got {reduction_db!r}")
        try:
            _, self.delay_size = stream_denoise_geometry(block_size, hop)
        except ValueError as e:
            raise ValueError(f"StreamDenoise: {e}") from None
        self.a_s, self.a_n, self.clamp, self.beta, self.warm = denoise_constants(hop, strength, smooth_ms, adapt_s, clamp, warmup_ms)
        self.n_streams, self.block_size, self.hop = n_streams, block_size, hop
        self.strength, self.smooth_ms, self.adapt_s, self.warmup_ms = float(strength), float(smooth_ms), float(adapt_s), float(warmup_ms)
        self.device = gpu_device(device, "StreamDenoise: the reduction and the state live on the GPU, where the suppressor's kernel runs")
        self.reduction_db = torch.tensor(red, dtype=torch.float32, device=self.device)
        allocate(self, DENOISE_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in: (n_streams, block_size, hop, a_s, a_n, clamp, beta, warm)"""
        return (self.n_streams, self.block_size, self.hop, self.a_s, self.a_n, self.clamp, self.beta, self.warm)

    def reset(self, streams=None):
        """Put every stream, or the listed ones, back at the start: empty tails, no estimate, no frame counted - so the warm-up runs again.
        In-place ops on the state tensors, so it works between replays of a captured graph, which reads them when it runs."""
        reset(self, DENOISE_STATE, streams)


class StreamLoudness:
    """The loudness envelope match of a set of streams that advance in lock step (tvc_stream_loudness_f32; its definition is in
    tinyvc_hip.h; 1 - RVC's rms_mix_rate): behind SOLA, every emitted block is scaled, sub-frame by sub-frame, by (Es / Eo)^(share / 2) -
    Es the mean power of the INPUT samples the block was converted from, Eo that of the block itself, each over the last 2 * smooth + 1
    sub-frames of the stream - so a speaker who drops to a murmur comes back as a murmur.  The gain trails the offline one
    (convert's loudness) by `smooth` sub-frames.  It never feeds back: the SOLA buffer and the window stay as they are.
      share [S]          fp32 on the device, read when a block runs and clamped to [0, 1] there: `stage.share.fill_(...)` / `copy_(...)` moves
                         it between blocks; 0 = the stream without the stage, bit for bit (the envelopes are still followed, so a share
                         raised later starts warm)
      sub_frame, smooth  24 kHz samples (a multiple of 4 that divides block_size) and sub-frames each side (0 .. 32); `window` = 2 * smooth + 1
      floor_db           powers below it (dB re full scale) count as it: silence is not amplified
      boost_db, cut_db   the most a sub-frame is turned up and down by (>= 0)
      src_ring, out_ring [S, window] fp64, frames [S] int64, gain [S] fp32      the state the next block starts from; gain_db [S]: the last gain in dB
    The defaults are guesses: nobody has listened to them yet.  Every argument is checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, block_size, share=1.0, sub_frame=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0, device=None):
        for x, name in ((n_streams, "n_streams"), (block_size, "block_size")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"StreamLoudness: {name} must be an integer >= 1, got {x!r}")
        rows = _db_rows(share, n_streams, f"StreamLoudness: share must be a number in [0, 1] or one per stream ({n_streams}), got {share!r}")
        if not all(0.0 <= v <= 1.0 for v in rows):
            raise ValueError(f"StreamLoudness: share must be a number in [0, 1] or one per stream ({n_streams}), got {share!r}")
        try:
            _, self.window, _ = loudness_geometry(block_size, sub_frame, smooth, stream_block=True)
        except ValueError as e:
            raise ValueError(f"StreamLoudness: {e}") from None
        self.floor_db, self.boost_db, self.cut_db = loudness_levels(floor_db, boost_db, cut_db, "StreamLoudness")
        self.n_streams, self.block_size, self.sub_frame, self.smooth = n_streams, block_size, int(sub_frame), int(smooth)
        self.device = gpu_device(device, "StreamLoudness: the share and the state live on the GPU, where the stage's kernel runs")
        self.share = torch.tensor(rows, dtype=torch.float32, device=self.device)
        allocate(self, LOUDNESS_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in: (n_streams, block_size, sub_frame, smooth, floor_db, boost_db, cut_db)"""
        return (self.n_streams, self.block_size, self.sub_frame, self.smooth, self.floor_db, self.boost_db, self.cut_db)

    def reset(self, streams=None):
        """Put every stream, or the listed ones, back at the start: empty envelopes, no sub-frame seen, gain 1 (the next block's first
        sub-frame is flat at its own gain).  In-place ops on the state tensors, so it works between replays of a captured graph."""
        reset(self, LOUDNESS_STATE, streams)


DOOR_CEILING_DB = -0.001      # the highest ceiling a limiter in front of a door may take: the int16 conversion wraps above 32767 / 32768 (-0.000265 dB)


class StreamLimiter:
    """The look-ahead peak limiter of a set of streams that advance in lock step (tvc_stream_limit_f32; its definition is in tinyvc_hip.h):
    the last stage of a block, behind the gate and in front of the door's output side.  A gain that falls at once, one sub-frame ahead of a
    peak, and rises linearly over release_size keeps every sample at or below the stream's ceiling - exactly, not as a tuning claim.  The
    stage holds one sub-frame back: it delays by `delay_size` = sub_frame samples.
      ceiling [S]     fp32 on the device, a LINEAR amplitude read when a block runs (NaN, <= 0 and inf: off); `set_ceiling_db(x, streams)`
                      converts dBFS on the host and copies, `stage.ceiling.fill_(...)` / `copy_(...)` takes linear values as they are
      ceiling_db      the start: a number of dBFS or one per stream (inf: off)
      sub_frame, release_size   24 kHz samples: the look-ahead and attack (a multiple of 4 that divides block_size; 24 = 1 ms), and the
                      time a gain of 0 takes back to 1 (1 .. 4096 whole sub-frames)
      drive_db        a gain in front of the limiter
      tail [S, sub_frame], peak [S], gain [S] fp32     the state the next block starts from; reduction_db [S]: the last block's deepest gain in dB
    Two limits of the guarantee.  A ceiling above 32767 / 32768 still wraps in a door's int16 conversion: streams with a door refuse a
    ceiling_db above -0.001 dB (`max_ceiling_db`, which set_ceiling_db holds too; a linear value written into `ceiling` directly is the
    caller's).  And a resampling door interpolates between samples and can overshoot the ceiling: the -1 dB default is margin, not proof.
    The defaults are guesses: nobody has listened to them yet.  Every argument is checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, block_size, ceiling_db=-1.0, sub_frame=24, release_size=2400, drive_db=0.0, device=None):
        for x, name in ((n_streams, "n_streams"), (block_size, "block_size")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"StreamLimiter: {name} must be an integer >= 1, got {x!r}")
        self.max_ceiling_db = None
        rows_db, rows = self._ceilings(ceiling_db, n_streams)
        self.sub_frame, self.release, self.drive_db = limiter_settings(sub_frame, release_size, drive_db, "StreamLimiter", block_size)
        self.n_streams, self.block_size, self.release_size, self.delay_size = n_streams, block_size, int(release_size), self.sub_frame
        self.device = gpu_device(device, "StreamLimiter: the ceilings and the state live on the GPU, where the stage's kernel runs")
        self.ceiling = torch.tensor(rows, dtype=torch.float32, device=self.device)
        self.ceiling_db = rows_db      # what the host last set, per stream: a value written into `ceiling` directly is not seen here
        allocate(self, LIMITER_STATE, self.device)

    def _ceilings(self, x, n):
        """ceilings in dBFS as given - a number or n of them - -> (n values in dB, the same as linear amplitudes); ValueError"""
        rows_db = _db_rows(x, n, f"StreamLimiter: ceiling_db must be a number of dBFS (inf: no limit) or one per stream ({n}), got {x!r}")
        if self.max_ceiling_db is not None and max(rows_db) > self.max_ceiling_db:
            raise ValueError(f"StreamLimiter: ceiling_db = {max(rows_db):g} is above {self.max_ceiling_db:g}: these streams end in a door, whose int16 "
                             "conversion wraps every sample above 32767 / 32768")
        return rows_db, [limit_ceiling(v, "StreamLimiter") for v in rows_db]

    def set_ceiling_db(self, x, streams=None):
        """Move the ceiling of every stream, or of the listed ones, to x dBFS (a number, or one per stream moved): converted to linear on the
        host, in double, and copied in place, so it works between replays of a captured graph."""
        idx = list(range(self.n_streams)) if streams is None else [int(i) for i in streams]
        rows_db, rows = self._ceilings(x, len(idx))
        self.ceiling.index_copy_(0, torch.as_tensor(idx, dtype=torch.int64, device=self.device), torch.tensor(rows, dtype=torch.float32, device=self.device))
        for i, v in zip(idx, rows_db):
            self.ceiling_db[i] = v

    def params(self):
        """the host values a captured block bakes in: (n_streams, block_size, sub_frame, release in sub-frames, drive_db)"""
        return (self.n_streams, self.block_size, self.sub_frame, self.release, self.drive_db)

    def reset(self, streams=None):
        """Put every stream, or the listed ones, back at the start: nothing held back, gain 1.  The ceilings stay.  In-place ops on the
        state tensors, so it works between replays of a captured graph."""
        reset(self, LIMITER_STATE, streams)


class BatchedStreamInfer:
    """`target`: one index for every stream ([1, 768, N]) or one per stream ([S, 768, N], or a list of S [1, 768, N_s] tensors), prepared
    once and cached on those tensors - or a feature_retrieval.Blend of several (its weights are read on the device when a block runs:
    `blend.weights.copy_(...)` between blocks moves the mix without a new graph capture); `pitch_shift`: a float or one per stream.
    `auto_pitch` (convert's: True, a register in Hz, or a [S] / [1] device tensor that is read when a block runs): every block moves each
    stream's register - the lower median of its last voiced frames, tracked on the device by `pitch_track` (a feature_retrieval.PitchTrack;
    built in init_buffer when not given: the block's own frames, last_dilay_size before the end of the buffer, are the new ones) - onto
    the target's; `pitch_shift` is the offset on top and `last_pitch_shift` [S] the shift the latest block applied, on the device.
    `alpha` (convert's: a float, one per stream, or a [S] / [1] fp32 device tensor): the share of each stream's own content features kept in
    the match, held as `self.alpha`, a [S] device tensor read when a block runs - `stream.alpha.fill_(...)` / `copy_(...)` between blocks
    moves it without a new graph capture; None (the default) is the plain match.
    `protect` (convert's, in alpha's forms; the keyword behind alpha): how far that share rises on the unvoiced frames of each window's own f0, held as
    `self.protect`, a [S] device tensor like `self.alpha` (`stream.protect.fill_(...)` / `copy_(...)` replay the same graph); with or without
    alpha; None (the default) is the stream as it was.
    `k` / `match_width` (convert's: an int in 1 .. 4 / a width >= 0 in cosine units, one per stream, or an int32 / fp32 [S] / [1] device
    tensor): the weighted match - every frame the mean over its k nearest index rows, weighted by their similarities -, held as `self.k`
    and `self.match_width`, [S] device tensors read when a block runs: `stream.k.fill_(1)` / `stream.match_width.fill_(...)` between blocks
    replay the same captured graph (their addresses are part of the graph key).  None for both (the default) is the stream as it was.
    `continuity` (convert's: a weight >= 0, one per stream, or an fp32 [S] / [1] device tensor): the match along a path, held as
    `self.continuity`, a [S] device tensor like `self.match_width` (`stream.continuity.fill_(...)` replays the same graph).  Every window
    decodes a path of its own over its frames; nothing is carried from window to window.  None (the default) is the stream as it was.
    `f0_estimation` (convert's): 'viterbi' or a feature_retrieval.PitchPath decodes every window's pitch as one path over its own frames
    (each window afresh unless f0_carry is set; the window's left context is what steadies the emitted frames); held as
    `self.f0_estimation`, and its settings - host values baked into the launch - are part of the graph key.  Every other name is ignored.
    `f0_carry` (with a pitch path; block_size in whole 480-sample frames): True carries the path's scores from block to block - the window
    advances by block_size / 480 frames, so the best-predecessor values of that frame of one window are the prior of the next window's
    first frame, the forward recursion of an online Viterbi - in `pitch_carry`, a feature_retrieval.PitchCarry built in init_buffer (or the
    one given here); `stream.pitch_carry.reset([i])` between blocks starts stream i's path afresh and keeps a captured graph.  False (the
    default) is the stream as it was, launch for launch.  Every window has logits of its own, so the carried scores are a prior, not the
    decode of any one tensor; nobody has listened.
    `tune` (block_size in whole 480-sample frames; refused with the reason otherwise): pitch correction, convert's `tune` - a
    feature_retrieval.PitchSnap or a string such as "A minor" - on the f0 every window's decoder reads; held as `self.tune`, with the note and
    the smoothed ratio of every stream travelling from window to window in `self.tune_carry`, a feature_retrieval.SnapCarry built in
    init_buffer.  `stream.tune.notes.copy_(...)`, `stream.tune.strength.fill_(...)`, `stream.tune.set_scale(...)` within the same range and
    `stream.tune_carry.reset([i])` between blocks replay the same captured graph; the host settings (hysteresis, retune, the range) and the
    addresses are part of the graph key.  Every window decodes an f0 of its own, so the state is a prior, not the run over one tensor.
    None (the default) is the stream as it was, launch for launch.  The defaults are guesses: nobody has listened.
    `door` (a StreamDoor of the same n_streams and block_size): audio_callback_pcm takes the clients' int16 blocks at the door's rates.
    `gate` (a StreamGate of the same n_streams and block_size): every emitted block goes through the noise gate, one launch behind SOLA (and
    in front of the door), driven by the input window and `last_shift` on the device; the SOLA buffer and the window stay ungated.
    `gate.threshold_db.fill_(...)` / `copy_(...)` and `gate.reset(...)` between blocks keep a captured graph; None (the default) is the
    ungated stream, launch for launch.
    `denoise` (a StreamDenoise of the same n_streams and block_size): every block goes through the spectral suppressor, one launch in front of
    the window (behind the door's input side), so the converter, the pitch tracker and the gate see the suppressed signal; it adds
    `denoise.delay_size` samples of latency.  `denoise.reduction_db.fill_(...)` / `copy_(...)` and `denoise.reset(...)` between blocks keep a
    captured graph; None (the default) is the stream without it, launch for launch.
    `loudness` (a StreamLoudness of the same n_streams and block_size): every emitted block follows the loudness envelope of the input it was
    converted from, one launch behind SOLA and in front of the gate (and the door), driven by the input window and `last_shift` on the
    device; the SOLA buffer and the window stay as they are.  `loudness.share.fill_(...)` / `copy_(...)` and `loudness.reset(...)` between
    blocks keep a captured graph; None (the default) is the stream without it, launch for launch.
    `limiter` (a StreamLimiter of the same n_streams and block_size): a look-ahead peak limiter, the last launch of a block - behind the gate,
    in front of the door's output side -, so that nothing leaves above a stream's ceiling; it adds `limiter.delay_size` samples of latency,
    and with a door it takes no ceiling above -0.001 dBFS.  `limiter.ceiling.fill_(...)`, `limiter.set_ceiling_db(...)` and
    `limiter.reset(...)` between blocks keep a captured graph; None (the default) is the stream without it, launch for launch.
    `crossfade_size`, `sola_search_size`, `last_delay_size` (kept as the attribute `last_dilay_size`, the reference's spelling): the tail's
    geometry in 24 kHz samples, within engine.sola_geometry's limits; `latency_samples` / `latency_seconds` give the resulting range.  The
    attributes are plain, as in the reference: one changed after construction takes effect at the next init_buffer(), which checks them again
    and recomputes input_size; until then every block is refused (ValueError), never run against buffers, a window or a tracker lag that no
    longer match.  A window that is not whole 480-sample frames is padded by convert at its end (`pad_size`): the latency is that much
    shorter than the three sizes say, and a look-ahead shorter than the pad is refused."""

    def __init__(self, generator: Generator, n_streams=1, target=None, pitch_shift=0., device=None,
                 block_size=1920, extra_size=0, use_phase_vocoder=False, f0_estimation="default", use_graph=False, alpha=None, protect=None, k=None, match_width=None, continuity=None, denoise=None, loudness=None, gate=None, limiter=None, f0_carry=False, tune=None, door=None,
                 crossfade_size=SOLA_CROSS, sola_search_size=SOLA_SEARCH, last_delay_size=SOLA_DELAY, auto_pitch=None, pitch_track=None):
        self.input_size, _ = check_window(block_size, extra_size, crossfade_size, sola_search_size, last_delay_size,
                                           auto_pitch is not None and auto_pitch is not False)
        self.f0_carry = check_f0_carry(f0_carry, f0_estimation, block_size, n_streams)      # refused here, before anything is allocated
        self.pitch_carry = self.f0_carry if isinstance(self.f0_carry, PitchCarry) else None
        self.tune = check_stream_tune(tune, block_size)
        self.tune_carry = None
        share = resolve_alpha(alpha, n_streams) if alpha is not None else None      # refused here, before anything is allocated
        guard = resolve_protect(protect, n_streams) if protect is not None else None
        near = resolve_match_k(k, n_streams) if k is not None else None
        wide = resolve_match_width(match_width, n_streams) if match_width is not None else None
        along = resolve_continuity(continuity, n_streams, wide) if continuity is not None else None
        self.n_streams, self.block_size = n_streams, block_size
        self.door, self.gate, self.denoise, self.loudness, self.limiter = (self._fits(name, stage) for name, stage in (
            ("door", door), ("gate", gate), ("denoise", denoise), ("loudness", loudness), ("limiter", limiter)))
        self._bound_ceiling()
        self.auto_pitch = auto_pitch if auto_pitch is not False else None
        self.pitch_track = pitch_track
        self._own_track = pitch_track is None
        if pitch_track is not None and self.auto_pitch is None:
            raise ValueError("pitch_track needs auto_pitch: the tracker finds the register the automatic shift starts from")
        if self.auto_pitch is not None and block_size % 480:
            raise ValueError(f"auto_pitch: block_size = {block_size} is not a whole number of 480-sample frames")
        self.last_pitch_shift = None
        self.generator = generator
        self.target = target
        self.pitch_shift = pitch_shift
        self.device = torch.device(device) if device is not None else generator._module_device()
        # the streams' shares of their own content features: a [S] device tensor every block reads when it runs, or None (the plain match)
        self.alpha = alpha_rows(share, n_streams, self.device) if share is not None else None
        self.protect = protect_rows(guard, n_streams, self.device) if guard is not None else None      # ... and their rise on unvoiced frames, likewise
        # the weighted match: k and the similarity width of every stream, [S] device tensors read when a block runs, or None (four rows, equal weights)
        self.k = match_k_rows(near, n_streams, self.device) if near is not None else None
        self.match_width = match_width_rows(wide, n_streams, self.device) if wide is not None else None
        self.continuity = continuity_rows(along, n_streams, self.device) if along is not None else None      # the match along a path, likewise
        self.extra_size = extra_size
        self.sola_search_size = sola_search_size
        self.last_dilay_size = last_delay_size          # (sic) the reference's attribute name, stream.py:49
        self.crossfade_size = crossfade_size
        self.use_phase_vocoder = use_phase_vocoder
        self.f0_estimation = f0_estimation
        self.last_shift = None
        # use_graph: after two eager warm-up blocks the whole per-block pipeline (buffer roll, noise draw,
        # convert, SOLA) is captured once into a HIP graph and replayed per block: ~170 launches become one.
        self.use_graph = use_graph
        self._graph = None
        self._calls = 0

    @property
    def latency_samples(self):
        """(min, max) 24 kHz samples between the first sample of the newest input block and the first sample of the block emitted for it:
        crossfade + delay .. crossfade + search + delay, by the lag the search picks, LESS the pad of a window that is not whole 480-sample
        frames (`pad_size`: convert pads the window at its end, the tail counts from the end of the padded conversion, so that much of the
        look-ahead is padding and the block leaves that much earlier), PLUS the suppressor's delay_size when there is one; the door's two
        and the limiter's; the door's two filters come on top in latency_seconds"""
        _, lo, hi = sola_geometry(self.block_size, self.crossfade_size, self.sola_search_size, self.last_dilay_size)
        extra = sum(stage.delay_size for stage in (self.denoise, self.limiter) if stage is not None)
        return lo - self.pad_size + extra, hi - self.pad_size + extra

    @property
    def pad_size(self):
        """samples of zero padding convert puts behind the window to make it whole frames"""
        return -self.input_size % FRAME

    @property
    def latency_seconds(self):
        """latency_samples in seconds, plus the door's latency_seconds when there is a door; the time to collect a block is not included"""
        extra = self.door.latency_seconds if self.door is not None else 0.0
        lo, hi = self.latency_samples
        return lo / MODEL_RATE + extra, hi / MODEL_RATE + extra

    def _fits(self, name, stage):
        """`stage` (a door, a gate, a suppressor, a loudness match, a limiter, or None) when it was built for these streams; ValueError otherwise"""
        if stage is not None and (stage.n_streams, stage.block_size) != (self.n_streams, self.block_size):
            raise ValueError(f"{name}: built for {stage.n_streams} streams of {stage.block_size}-sample blocks, the streams are "
                             f"{self.n_streams} of {self.block_size}")
        return stage

    def _bound_ceiling(self):
        """a limiter in front of a door: its ceilings stay at or below DOOR_CEILING_DB, now and in set_ceiling_db (ValueError)"""
        if self.limiter is not None and self.door is not None:
            if max(self.limiter.ceiling_db) > DOOR_CEILING_DB:
                raise ValueError(f"limiter: ceiling_db = {max(self.limiter.ceiling_db):g} is above {DOOR_CEILING_DB:g}: the door's int16 conversion wraps every "
                                 "sample above 32767 / 32768, so such a ceiling bounds nothing")
            self.limiter.max_ceiling_db = DOOR_CEILING_DB

    def _stages(self):
        """the stages of these streams that keep state on the device, in block order: (name, stage, its table in stream_state)"""
        every = (("track", self.pitch_track if self.auto_pitch is not None else None, TRACK_STATE), ("door", self.door, DOOR_STATE),
                 ("denoise", self.denoise, DENOISE_STATE), ("carry", self.pitch_carry, CARRY_STATE), ("tune_carry", self.tune_carry if self.tune is not None else None, SNAP_STATE),
                 ("loudness", self.loudness, LOUDNESS_STATE),
                 ("gate", self.gate, GATE_STATE), ("limiter", self.limiter, LIMITER_STATE))
        return [s for s in every if s[1] is not None]

    def init_buffer(self):
        # the attributes as they stand now (plain attributes, as in the reference): checked as in the constructor, the window follows them,
        # and _step holds every later block against what was seen here
        self.input_size, _ = check_window(self.block_size, self.extra_size, self.crossfade_size, self.sola_search_size, self.last_dilay_size,
                                           self.auto_pitch is not None)
        for name in ("door", "gate", "denoise", "loudness", "limiter"):      # (before anything is allocated) the stages against the attributes as they stand now
            self._fits(name, getattr(self, name))
        self._bound_ceiling()
        self.f0_carry = check_f0_carry(self.f0_carry, self.f0_estimation, self.block_size, self.n_streams)
        self.tune = check_stream_tune(self.tune, self.block_size)
        if self.gate is not None:
            check_gate_lookahead(self.gate.lookahead_size, self.crossfade_size, self.last_dilay_size, self.pad_size)
        self._geometry = self._attributes()
        self.fade_in_window, self.fade_out_window = _fade_windows(self.crossfade_size, self.device)
        self.input_wav = torch.zeros(self.n_streams, self.input_size, device=self.device)
        self.sola_buffer = torch.zeros(self.n_streams, self.crossfade_size, device=self.device)
        self._graph = None
        self._calls = 0
        if self.auto_pitch is not None and self._own_track:      # the block's own frames: they have their full right context and are the audio about to be played
            self.pitch_track = PitchTrack(self.n_streams, self.block_size // 480, self.last_dilay_size // 480, device=self.device)
        if self.f0_carry is True:      # the window advances by the block's frames: that frame of this window is the next one's first
            self.pitch_carry = PitchCarry(self.n_streams, self.block_size // FRAME, device=self.device)
        else:
            self.pitch_carry = self.f0_carry
        # the correction's state: what it holds behind the block's last new frame of one window is where frame 0 of the next starts
        self.tune_carry = SnapCarry(self.n_streams, self.block_size // FRAME, device=self.device) if self.tune is not None else None
        if self.tune is not None:
            self.tune.bind(self.device, self.n_streams)      # the table and the strengths: tensors every block reads when it runs
        if self.door is not None:
            self.door.prepare(self.generator.engine(self.device))
        for _, stage, _ in self._stages():
            stage.reset()

    def _attributes(self):
        return (self.block_size, self.crossfade_size, self.sola_search_size, self.last_dilay_size, self.input_size)

    def _tune_kw(self):
        """convert's keywords of the pitch correction: none without `tune`, so the call is the one it was"""
        return {"tune": self.tune, "tune_carry": self.tune_carry} if self.tune is not None else {}

    def _step(self, blocks, noise_angle):
        # torch.roll + slice assignment of the reference (stream.py:69-70), in place on a fixed buffer, one launch
        if self.denoise is not None:      # in front of everything else: the window holds the suppressed signal, denoise.delay_size samples late
            blocks = self.generator.engine(self.device).stream_denoise(blocks.contiguous(), self.denoise)
        self.generator.engine(self.device).stream_push(self.input_wav, blocks)
        if noise_angle is None and self.use_graph:
            # a captured step bakes kernel arguments in: the library's seeded draw would replay ONE seed for every block.  torch's
            # generator is graph-safe (its offset advances per replay), so the graph path keeps the reference's torch.rand draw
            from ..tinyvc import Decoder
            noise_angle = Decoder.draw_noise_angle(self.n_streams, -(-self.input_size // 480), self.device)      # (convert pads the window to whole frames)
        pshift = None
        if self.auto_pitch is None:
            y = self.generator.convert(self.input_wav, self.target, self.pitch_shift, device=self.device,
                                       f0_estimation=self.f0_estimation, noise_angle=noise_angle, alpha=self.alpha, protect=self.protect,
                                       carry=self.pitch_carry, k=self.k, match_width=self.match_width, continuity=self.continuity, **self._tune_kw())
        else:
            y, pshift = self.generator.convert(self.input_wav, self.target, self.pitch_shift, device=self.device, f0_estimation=self.f0_estimation,
                                               noise_angle=noise_angle, auto_pitch=self.auto_pitch, return_shift=True, track=self.pitch_track,
                                               alpha=self.alpha, protect=self.protect, carry=self.pitch_carry, k=self.k, match_width=self.match_width,
                                               continuity=self.continuity, **self._tune_kw())
        eng = self.generator.engine(self.device)
        out, shift = eng.sola(y, self.sola_buffer, self.fade_in_window, self.block_size, self.use_phase_vocoder, want_shift=True,
                              crossfade=self.crossfade_size, search=self.sola_search_size, delay=self.last_dilay_size)
        # y[Ly - block - crossfade - search - delay + shift + j] became out[j], and convert keeps the window's time axis (padding at the end)
        base = y.shape[1] - self.block_size - self.crossfade_size - self.sola_search_size - self.last_dilay_size
        if self.loudness is not None:      # in front of the gate: the gate's fades stay what they are
            eng.stream_loudness(self.input_wav, out, shift, self.loudness, base, out=out)
        if self.gate is not None:
            eng.stream_gate(self.input_wav, out, shift, self.gate, base, out=out)
        if self.limiter is not None:      # last: whatever the stages before it did to the level, nothing leaves above the ceiling
            out = eng.stream_limit(out, self.limiter)
        return out, shift, pshift

    def _step_pcm(self, pcm, noise_angle):
        # the whole block from client int16 to client int16: door in, _step (convert, SOLA, loudness, gate, limiter), door out
        eng = self.generator.engine(self.device)
        out, shift, pshift = self._step(self.door.push(eng, pcm), noise_angle)
        return self.door.pull(eng, out), shift, pshift

    def _graph_key(self):
        """Everything a captured step bakes in as raw device pointers: the packed weights (re-packed - and the old arena
        freed - when a parameter changes), the engine's scratch workspace (re-allocated when another call needs a bigger
        one), the prepared index riding on `target`, plus the scalars captured by value.  Every stage present - the
        tracker, the door, the suppressor (denoise), the pitch path's carry, the pitch correction's state, the loudness match, the gate, the limiter - adds (its name, WHERE the tensors of its table in stream_state live, its
        params()): the table lists every tensor whose pointer reaches the library, so none can be passed on and left out here.  With
        auto_pitch also WHERE the target registers live, with alpha / protect where the shares live.  Never a value: the kernels read those at replay,
        so a reset(), registers.copy_(...), threshold_db.fill_(...) or a stream's history advancing keeps the graph.  The tail's geometry is
        baked into its two launches, so it is part of the key."""
        eng = self.generator.engine(self.device)          # re-packs the weights first if a parameter changed
        ws = eng._ws
        form, tgts = target_form(self.target)      # every blob's tensor
        wkey = 0
        if form == "blend":      # WHERE the weights live - not their version or values: the kernels read them at replay
            wkey = self.target.resolve(self.n_streams, self.device, self.generator._input_device)[2].data_ptr()
        shift, shifts = pitch_shifts(self.pitch_shift, self.n_streams)
        shifts = shift if shifts is None else tuple(shifts)
        tkey = tuple((name, addresses(stage, table), stage.params()) for name, stage, table in self._stages())
        if self.auto_pitch is not None:
            regs = resolve_auto_pitch(self.auto_pitch, self.target, self.n_streams)
            tkey += (("target_f0", regs if isinstance(regs, float) else tuple(r.data_ptr() for r in regs)),)
        if self.alpha is not None:      # WHERE the shares live, not their values: alpha.fill_(...) / copy_(...) keeps the graph
            tkey += (("alpha", self.alpha.data_ptr()),)
        if self.protect is not None:
            tkey += (("protect", self.protect.data_ptr()),)
        if self.k is not None:      # likewise: k.fill_(...) / match_width.fill_(...) keep the graph
            tkey += (("k", self.k.data_ptr()),)
        if self.match_width is not None:
            tkey += (("match_width", self.match_width.data_ptr()),)
        if self.continuity is not None:
            tkey += (("continuity", self.continuity.data_ptr()),)
        path = resolve_f0_estimation(self.f0_estimation)
        if path is not None:      # the pitch path's settings ARE values: host numbers baked into the launch, so another PitchPath is another graph
            tkey += (("f0_estimation", path.params()),)
        if self.tune is not None:      # the correction's host settings are values; its table and strengths are read at replay: WHERE they live
            tkey += (("tune", self.tune.params(), self.tune.notes.data_ptr(), self.tune.strength.data_ptr()),)
        return (eng.weights_key, ws.data_ptr() if ws is not None else 0, ws.numel() if ws is not None else 0,
                tuple((id(t), t._version, t.data_ptr()) for t in tgts), wkey, shifts, bool(self.use_phase_vocoder),
                (self.crossfade_size, self.sola_search_size, self.last_dilay_size)) + tkey

    @torch.no_grad()
    def audio_callback(self, blocks, noise_angle=None):
        """blocks [S, block_size] -> converted blocks [S, block_size]."""
        return self._callback(blocks, noise_angle, False)

    @torch.no_grad()
    def audio_callback_pcm(self, pcm, noise_angle=None):
        """The clients' blocks through the door: pcm [S, door.chunk_in] int16 at door.in_rate -> int16 [S, door.chunk_out] at door.out_rate.
        Door in (int16 -> fp32, input gain, resample to 24 kHz), the block of audio_callback, door out (resample, output gain, int16); with
        use_graph all of it is one captured graph."""
        if self.door is None:
            raise ValueError("audio_callback_pcm needs a door: BatchedStreamInfer(..., door=StreamDoor(n_streams, in_rate, ...))")
        if pcm.dtype != torch.int16 or tuple(pcm.shape) != (self.n_streams, self.door.chunk_in):
            raise ValueError(f"audio_callback_pcm: int16 [{self.n_streams}, {self.door.chunk_in}] blocks at {self.door.in_rate} Hz, got "
                             f"{pcm.dtype} {tuple(pcm.shape)}")
        return self._callback(pcm, noise_angle, True)

    def _callback(self, blocks, noise_angle, pcm):
        if self._attributes() != getattr(self, "_geometry", None):      # before anything runs or is captured
            raise ValueError(f"block_size / crossfade_size / sola_search_size / last_dilay_size / input_size are {self._attributes()}, init_buffer() saw "
                             f"{getattr(self, '_geometry', None)}: the buffers, the window and the tracker's lag follow them only there - call init_buffer()")
        step = self._step_pcm if pcm else self._step
        blocks = blocks.to(self.device)
        self._calls += 1
        if not self.use_graph or self._calls <= 2:
            out, self.last_shift, self.last_pitch_shift = step(blocks, noise_angle)
            return out
        key = self._graph_key()
        if self._graph is not None and key != self._graph[0]:
            self._graph = None        # stale pointers inside the captured graphs: drop them and capture again
        if self._graph is None:
            self._graph = (key, {})
            self._g_in = torch.zeros(self.n_streams, self.block_size, device=self.device)
            self._g_pcm = torch.zeros(self.n_streams, self.door.chunk_in, dtype=torch.int16, device=self.device) if self.door is not None else None
            self._g_angle = torch.zeros(self.n_streams, 961, -(-self.input_size // 480), device=self.device)
        inject = noise_angle is not None      # injected phases replay from a static buffer; otherwise the draw is part of the graph
        g_in = self._g_pcm if pcm else self._g_in
        slot = ("pcm", inject) if pcm else inject
        graphs = self._graph[1]
        if slot not in graphs:
            g_in.copy_(blocks)
            if inject:
                self._g_angle.copy_(noise_angle)
            # capture changes no state: the buffer roll, convert and SOLA (and the door's two launches) are recorded, not run
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                res = step(g_in, self._g_angle if inject else None)
            graphs[slot] = (g, res)
            if self._graph_key() != key:      # the capture itself grew the workspace: what it recorded is already stale
                self._graph = None
                out, self.last_shift, self.last_pitch_shift = step(blocks, noise_angle)
                return out
        g_in.copy_(blocks)
        if inject:
            self._g_angle.copy_(noise_angle)
        g, (g_out, g_shift, g_pshift) = graphs[slot]
        g.replay()
        self.last_shift, self.last_pitch_shift = g_shift, g_pshift
        return g_out.clone()


class StreamInfer(BatchedStreamInfer):
    """Single stream with the reference's constructor and 1-D buffers (stream.py:31-57)."""

    def __init__(self, generator: Generator, target=None, pitch_shift=0., device=torch.device("cpu"),
                 block_size=1920, extra_size=0, use_phase_vocoder=False, f0_estimation="default", use_graph=False, alpha=None, protect=None, k=None, match_width=None, continuity=None, denoise=None, loudness=None, gate=None, limiter=None, f0_carry=False, tune=None, door=None,
                 crossfade_size=SOLA_CROSS, sola_search_size=SOLA_SEARCH, last_delay_size=SOLA_DELAY, auto_pitch=None, pitch_track=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            dev = generator._module_device()     # the reference defaults to CPU; there is no CPU path here
        super().__init__(generator, n_streams=1, target=target, pitch_shift=pitch_shift, device=dev, block_size=block_size, extra_size=extra_size,
                         use_phase_vocoder=use_phase_vocoder, f0_estimation=f0_estimation, use_graph=use_graph, alpha=alpha, protect=protect, denoise=denoise, gate=gate,
                         limiter=limiter, door=door, crossfade_size=crossfade_size, sola_search_size=sola_search_size, last_delay_size=last_delay_size,
                         auto_pitch=auto_pitch, pitch_track=pitch_track, loudness=loudness, f0_carry=f0_carry, tune=tune, k=k, match_width=match_width, continuity=continuity)

    @torch.no_grad()
    def audio_callback(self, block, noise_angle=None):
        """block [block_size] -> converted block [block_size] (stream.py:68-96)."""
        return super().audio_callback(block[None], noise_angle)[0]

    @torch.no_grad()
    def audio_callback_pcm(self, pcm, noise_angle=None):
        """pcm [door.chunk_in] int16 -> int16 [door.chunk_out]."""
        return super().audio_callback_pcm(pcm[None], noise_angle)[0]
