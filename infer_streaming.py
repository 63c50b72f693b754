#!/usr/bin/env python3
"""Real-time voice conversion on an MI355X: the reference's `infer_streaming.py` entry point
(same flags, reference infer_streaming.py:18-35) on the HIP path.

With `pyaudio` installed and audio devices present it runs the reference's capture -> convert ->
playback loop.  GPU nodes have neither, so the same loop can be driven from files:

  python infer_streaming.py -encp enc.pt -decp dec.pt -idx index.pt \\
         --input-wav in.wav --output-wav out.wav [--streams 32]

`--blend PATH=W [PATH=W ...]` (extension) takes the place of `-idx` / `-t`: a weighted blend of up to four index files.

`--auto-pitch-from calib.wav` (extension) measures the speaker's pitch register ONCE from a calibration recording (the lower median of its
voiced f0, on the device) and fixes the session's pitch shift at -p + 12 log2(target register / speaker register); the target's register
comes from the index's `.f0.pt` sidecar (extract_index.py) or from the `-t` recording.  The shift does not move during the session.

`--auto-pitch` (extension) is the live form: every block, each stream's register - the lower median of its last `--auto-pitch-window`
seconds of voiced f0, tracked on the device - is moved onto the target's, no faster than `--auto-pitch-slew` semitones per second and only
once `--auto-pitch-warmup` seconds of voiced speech have been heard; `-p` is added on top.  No calibration recording, no host read per block.

`--resample` (extension) runs the audio device - or the file - at `-sr` for real: `-c` counts samples at that rate, every block is resampled
to the model's 24 kHz on the way in and back to `-sr` on the way out by a stateful resampler on the device (StreamDoor: the filter history
is carried per stream, so there is no transient at block edges), and `-ig` / `-og` are applied there.  The model block is c * 24000 / sr and
must be an integer made of whole resampling groups (44.1 kHz: multiples of 147 samples, e.g. -c 3528).  Without the flag `-sr` only opens the
device at that rate and the samples are taken for 24 kHz, as in the reference.

`--crossfade N --sola-search N --lookahead N` (extension) set the SOLA geometry the reference hard-codes (1920, 1920, 3840), in samples at
the model's 24 kHz.  A block's first sample is played crossfade + lookahead .. crossfade + sola-search + lookahead samples after the first
sample of the newest block came in (240 .. 320 ms at the defaults), plus the block itself: the latency is these three numbers, not compute.
Look-ahead is the right context the converter sees behind the block it emits; a shorter one trades that context for latency.

`--gate DB` (extension) puts a noise gate behind SOLA, on the device: a stream whose input falls below DB (mean power of a 10 ms sub-frame, dB
re full scale) for longer than `--gate-hold` fades to `--gate-range` (default: silence) over `--gate-release`, and opens again over
`--gate-attack` as soon as a sub-frame within `--gate-lookahead` of the one being played reaches DB; it stays open down to DB minus
`--gate-hysteresis`.  The gate reads the input window the converter already holds, aligned with the played block by SOLA's own lag, so the
look-ahead costs no latency.  Times are in milliseconds, rounded to whole 10 ms sub-frames.  The defaults are guesses: nobody has listened yet.

`--denoise DB` (extension) puts a spectral suppressor in front of the converter, on the device: steady noise under the speech (fan, room,
laptop microphone) is estimated per frequency bin - from the first `--denoise-warmup` of sound, then adapting over `--denoise-adapt` - and
every bin is turned down by up to DB where the estimate explains its power (`--denoise-strength`: the over-subtraction factor;
`--denoise-smooth`: the time constant of the power the gain follows).  The converter, the pitch tracker and the gate then see the cleaned
signal.  It costs 640 - `--denoise-hop` samples of latency (20 ms at hop 160, 13.3 ms at 320).  The defaults are guesses: nobody has listened yet.

`--loudness E` (extension; 1 - RVC's rms_mix_rate) makes every stream follow that share of its speaker's loudness envelope, on the device
behind SOLA and in front of the gate: each 10 ms sub-frame of a played block is scaled by (Es / Eo)^(E / 2), Es and Eo the mean powers of
the input the block was converted from and of the block itself over the last `--loudness-window`; powers below `--loudness-floor` count as
it, and a sub-frame is never turned up by more than `--loudness-boost` or down by more than `--loudness-cut`.  It adds no latency.  The
defaults are guesses: nobody has listened yet.

`--limit [DB]` (extension; bare: -1) ends every stream in a look-ahead peak limiter on the device, behind the gate and in front of the int16
conversion: no sample leaves above DB dBFS - exactly -, where without it a sample of 1.0 or more wraps to a full-scale click.  The gain
falls at once, 1 ms ahead of a peak, and rises linearly over `--limit-release`.  `-og` then becomes the limiter's drive: the gain is applied
in front of the limiter, not behind it.  It costs 1 ms of latency.  DB is at most -0.001 (above 32767 / 32768 the conversion wraps); with
--resample the filter on the way out can overshoot the ceiling between samples: -1 dB is margin, not proof.  The defaults are guesses:
nobody has listened yet.

`--streams S` feeds S copies of the input as S concurrent streams through one BatchedStreamInfer
(one batched convert + one SOLA launch per block) and reports the p50 / p95 block latency against the
real-time budget (chunk / 24 kHz = 80 ms for the default 1920-sample chunk).
"""
import argparse
import math
import sys
import time

import numpy as np
import torch

from tinyvc_amd import audio_io
from infer import load_generator, load_target
from tinyvc_amd.engine import limiter_drive, limiter_geometry, loudness_geometry, loudness_levels, sola_geometry, stream_denoise_geometry, stream_gate_geometry, stream_resample_geometry
from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDenoise, StreamDoor, StreamGate, StreamLimiter, StreamLoudness
from tinyvc_amd.module.infer.stream import DOOR_CEILING_DB, check_gate_lookahead, check_window, denoise_constants
from tinyvc_amd.module.tinyvc.feature_retrieval import (PitchTrack, add_alpha_argument, add_match_weight_argument, match_weight_keywords, add_continuity_argument, continuity_keywords, add_blend_argument, add_f0_arguments, alpha_keywords, f0_keywords,
                                                        add_f0_carry_argument, add_tune_arguments, f0_carry_keywords, tune_keywords,
                                                        pitch_register, semitones_between)

FRAMES_PER_SECOND = 50      # 24 kHz / 480 samples
GATE_SUB_FRAME = 240        # the gate's sub-frame: 10 ms at 24 kHz
DENOISE_DEFAULTS = dict(hop=160, strength=2.0, adapt_s=1.0, smooth_ms=40.0, warmup_ms=200.0)      # of --denoise-hop / -strength / -adapt / -smooth / -warmup
LOUDNESS_DEFAULTS = dict(window=50.0, floor=-60.0, boost=12.0, cut=40.0)      # of --loudness-window (ms) / -floor / -boost / -cut (dB)
LIMIT_SUB_FRAME = 24        # the limiter's sub-frame, its look-ahead and delay: 1 ms at 24 kHz
LIMIT_RELEASE_MS = 100.0    # the default of --limit-release
GATE_MS = dict(hold=200.0, attack=10.0, release=100.0, lookahead=20.0)      # the defaults of --gate-hold / -attack / -release / -lookahead


def build_parser():
    p = argparse.ArgumentParser(description="realtime inference")
    p.add_argument("-encp", "--encoder-path", default="./models/encoder.pt")
    p.add_argument("-decp", "--decoder-path", default="./models/decoder.pt")
    p.add_argument("-i", "--input", default=0, type=int)
    p.add_argument("-o", "--output", default=0, type=int)
    p.add_argument("-l", "--loopback", default=-1, type=int)
    p.add_argument("-idx", "--index", default="NONE")
    p.add_argument("-p", "--pitch-shift", default=0, type=float)
    p.add_argument("-t", "--target", default="target.wav")
    p.add_argument("--auto-pitch-from", default=None, metavar="WAV",
                   help="measure the speaker's median f0 once from this recording and fix the session's shift at -p + the semitones onto the target's register")
    p.add_argument("--auto-pitch", action="store_true",
                   help="live: keep every stream's median f0 (over --auto-pitch-window of its voiced history, tracked on the device) on the target's "
                        "register; -p is added on top.  The three defaults below are guesses: nobody has listened to them yet")
    p.add_argument("--auto-pitch-window", default=30.0, type=float, metavar="SECONDS", help="voiced history the register is the median of (at most 163 s)")
    p.add_argument("--auto-pitch-warmup", default=0.5, type=float, metavar="SECONDS", help="voiced speech heard before the automatic shift starts")
    p.add_argument("--auto-pitch-slew", default=6.0, type=float, metavar="SEMITONES_PER_SECOND", help="how fast the automatic shift may move; 0 = unlimited")
    add_blend_argument(p)      # --blend PATH=W [PATH=W ...] -> args.blend = (paths, weights)
    add_alpha_argument(p)      # --alpha A: keep that share of every stream's own content features in the match (stream.alpha, live on the device); --protect P (stream.protect)
    add_match_weight_argument(p)      # -k K --match-width W: the weighted match (stream.k / stream.match_width, live on the device)
    add_continuity_argument(p)      # --continuity C: the match along a path (stream.continuity, live on the device); every window a path of its own
    p.add_argument("-c", "--chunk", default=1920, type=int)
    p.add_argument("-e", "--extra", default=3840, type=int)
    p.add_argument("-d", "--device", default="cuda")
    p.add_argument("-sr", "--sample-rate", default=24000, type=int)
    p.add_argument("-ig", "--input-gain", default=0, type=float)
    p.add_argument("-og", "--output-gain", default=0, type=float)
    add_f0_carry_argument(p)      # --f0-carry: with -f0-est viterbi, the path's scores travel from block to block
    add_tune_arguments(p)         # --tune "KEY SCALE" and its settings: pitch correction on the f0 every window's decoder reads
    add_f0_arguments(p, choices=["default", "fcpe", "dio", "harvest", "viterbi"])      # viterbi: each window's pitch as one path (--f0-step .. --f0-refine)
    p.add_argument("--resample", action="store_true",
                   help="run the device (or file) at -sr and resample every block to the model's 24 kHz and back on the GPU; -c counts samples at -sr, "
                        "-ig / -og are applied by the same kernels")
    p.add_argument("--crossfade", default=1920, type=int, metavar="N", help="SOLA cross-fade length in 24 kHz samples: a multiple of 4 in 4 .. 1920")
    p.add_argument("--sola-search", default=1920, type=int, metavar="N", help="SOLA lag search range in 24 kHz samples: 0 .. 1920 (0 = a plain cross-fade)")
    p.add_argument("--lookahead", default=3840, type=int, metavar="N",
                   help="24 kHz samples of converted audio behind the emitted block (the reference's last_dilay_size): right context for the converter, "
                        "paid for in latency; with --auto-pitch a multiple of 480")
    p.add_argument("--gate", default=None, type=float, metavar="DB",
                   help="noise gate on the device behind SOLA: streams whose input stays below DB (dB re full scale, per 10 ms sub-frame) fade out; "
                        "--gate=-inf is an always-open gate.  Absent: no gate.  The defaults of the six flags below are guesses: nobody has listened yet")
    p.add_argument("--gate-hysteresis", default=None, type=float, metavar="DB", help="an open gate stays open down to --gate minus this (default 6)")
    p.add_argument("--gate-range", default=None, type=float, metavar="DB", help="gain of a closed gate, <= 0 (default -inf: silence)")
    p.add_argument("--gate-hold", default=None, type=float, metavar="MS", help=f"how long the gate outlasts the last loud sub-frame (default {GATE_MS['hold']:g})")
    p.add_argument("--gate-attack", default=None, type=float, metavar="MS", help=f"fade-in time, at least one sub-frame (default {GATE_MS['attack']:g})")
    p.add_argument("--gate-release", default=None, type=float, metavar="MS", help=f"fade-out time, at least one sub-frame (default {GATE_MS['release']:g})")
    p.add_argument("--gate-lookahead", default=None, type=float, metavar="MS",
                   help=f"how far ahead of the played sample the gate looks in the input it already holds: no added latency, at most "
                        f"--crossfade + --lookahead samples (default {GATE_MS['lookahead']:g})")
    p.add_argument("--denoise", default=None, type=float, metavar="DB",
                   help="spectral noise suppressor on the device in front of the converter: every frequency bin is turned down by up to DB where the "
                        "noise estimate explains its power (0: the delayed input).  Absent: no suppressor.  It adds 640 - --denoise-hop samples of "
                        "latency.  The defaults of the five flags below are guesses: nobody has listened yet")
    p.add_argument("--denoise-hop", default=None, type=int, choices=[160, 320], help="hop of the 640-sample frames: 20 ms or 13.3 ms of delay (default 160)")
    p.add_argument("--denoise-strength", default=None, type=float, metavar="X", help=f"over-subtraction factor, >= 0 (default {DENOISE_DEFAULTS['strength']:g})")
    p.add_argument("--denoise-adapt", default=None, type=float, metavar="S", help=f"time constant of the noise estimate in seconds (default {DENOISE_DEFAULTS['adapt_s']:g})")
    p.add_argument("--denoise-smooth", default=None, type=float, metavar="MS",
                   help=f"time constant of the smoothed power the gain follows, in milliseconds (default {DENOISE_DEFAULTS['smooth_ms']:g})")
    p.add_argument("--denoise-warmup", default=None, type=float, metavar="MS",
                   help=f"the first this many milliseconds of sound in a stream are taken for noise (default {DENOISE_DEFAULTS['warmup_ms']:g})")
    p.add_argument("--loudness", default=None, type=float, metavar="E",
                   help="make every stream follow this share (0 .. 1) of its speaker's loudness envelope, on the device behind SOLA and in front of the "
                        "gate (1 - RVC's rms_mix_rate; stage.share, live on the device).  Absent: the level the decoder gives.  The defaults of the "
                        "four flags below are guesses: nobody has listened yet")
    p.add_argument("--loudness-window", default=None, type=float, metavar="MS",
                   help=f"length of the trailing window both envelopes are taken over: an odd number of 10 ms sub-frames, at most 65 (default {LOUDNESS_DEFAULTS['window']:g})")
    p.add_argument("--loudness-floor", default=None, type=float, metavar="DB",
                   help=f"powers below this (dB re full scale) count as it: silence is not amplified (default {LOUDNESS_DEFAULTS['floor']:g})")
    p.add_argument("--loudness-boost", default=None, type=float, metavar="DB", help=f"the most a sub-frame is turned up by, >= 0 (default {LOUDNESS_DEFAULTS['boost']:g})")
    p.add_argument("--loudness-cut", default=None, type=float, metavar="DB", help=f"the most a sub-frame is turned down by, >= 0 (default {LOUDNESS_DEFAULTS['cut']:g})")
    p.add_argument("--limit", default=None, type=float, nargs="?", const=-1.0, metavar="DB",
                   help="end every stream in a look-ahead peak limiter on the device: no sample leaves above this ceiling (dBFS, at most -0.001; bare: -1), "
                        "where without it a sample of 1.0 or more wraps in the int16 conversion.  -og becomes the limiter's drive, in front of it; 1 ms of "
                        "latency (stage.ceiling, live on the device).  The defaults are guesses: nobody has listened yet")
    p.add_argument("--limit-release", default=None, type=float, metavar="MS",
                   help=f"the time a fully reduced gain takes back to 1: whole milliseconds, 1 .. 4096 (default {LIMIT_RELEASE_MS:g})")
    # file-driven operation (no audio devices on a GPU node)
    p.add_argument("--input-wav", default=None, help="read the microphone signal from this WAV instead of a device")
    p.add_argument("--output-wav", default=None, help="write the converted stream here")
    p.add_argument("--streams", default=1, type=int, help="number of concurrent streams to simulate")
    return p


def int16_blocks_from_wav(path, sample_rate, chunk, engine):
    """What `stream_input.read(chunk)` yields in the reference: int16 mono blocks at `sample_rate` (the file is resampled on the device,
    tvc_resample_f32, like every other resampling of the entry scripts; tinyvc_amd/resample.py is that kernel's host checker, not a second path)."""
    wf, sr = audio_io.load(path)
    wf = engine.resample(wf.mean(dim=0, keepdim=True).to(engine.device), sr, sample_rate)[0].cpu()
    pcm = (wf.clamp(-1, 1) * 32767).to(torch.int16).numpy()
    n = len(pcm) // chunk
    return [pcm[i * chunk:(i + 1) * chunk] for i in range(n)]


def check_resample(args):
    """--resample against -sr and -c, before anything is loaded: sys.exit with a message, or the model's block length at 24 kHz (None without
    the flag)"""
    if not args.resample:
        return None
    sr, c = args.sample_rate, args.chunk
    if sr <= 0 or c <= 0:
        sys.exit("infer_streaming.py: --resample: -sr and -c must be positive")
    orig = sr // math.gcd(sr, 24000)
    if c % orig:
        near = " or ".join(str(n) for n in (c // orig * orig, (c // orig + 1) * orig) if n > 0)
        sys.exit(f"infer_streaming.py: --resample: -c {c} at -sr {sr} is not a multiple of {orig}, the samples of one resampling group "
                 f"({sr} -> 24000 Hz); the nearest sizes that work: {near}")
    try:
        block, _, _ = stream_resample_geometry(sr, 24000, c)
        stream_resample_geometry(24000, sr, block)
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --resample: {e}")
    return block


def check_geometry(args, block=None):
    """--crossfade / --sola-search / --lookahead against the block (and -e, --auto-pitch; stream.check_window's rules), before anything is
    loaded: sys.exit with a message, or (latency_min, latency_max) in 24 kHz samples.  `block`: the model's block length when it is not -c (--resample)"""
    chunk = args.chunk if block is None else block
    try:
        _, pad = check_window(chunk, args.extra, args.crossfade, args.sola_search, args.lookahead, bool(args.auto_pitch))
        _, lo, hi = sola_geometry(chunk, args.crossfade, args.sola_search, args.lookahead)
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --crossfade {args.crossfade} --sola-search {args.sola_search} --lookahead {args.lookahead} -e {args.extra} with blocks of "
                 f"{chunk}: {e}")
    lo, hi = lo - pad, hi - pad      # a window that is not whole frames is padded behind its end: that much of the look-ahead is padding
    return lo, hi


def check_auto_pitch(args, block=None):
    """--auto-pitch against the other flags, before anything is loaded: sys.exit with a message, or the PitchTrack keywords (None without
    the flag).  `block`: the model's block length when it is not -c (--resample)"""
    if not args.auto_pitch:
        return None
    chunk = args.chunk if block is None else block
    if args.auto_pitch_from is not None:
        sys.exit("infer_streaming.py: --auto-pitch with --auto-pitch-from: the live tracker needs no calibration recording; pick one")
    if args.blend is not None:
        sys.exit("infer_streaming.py: --auto-pitch with --blend: a blend has no register of its own; use -p")
    if chunk <= 0 or chunk % 480:
        sys.exit(f"infer_streaming.py: --auto-pitch: -c {args.chunk} is not a whole number of 480-sample frames")
    if chunk // 480 > 256:
        sys.exit(f"infer_streaming.py: --auto-pitch: -c {args.chunk} is more than 256 frames per block")
    window = int(round(args.auto_pitch_window * FRAMES_PER_SECOND))
    if not 1 <= window <= 8192:
        sys.exit("infer_streaming.py: --auto-pitch-window: between 0.02 and 163.84 seconds")
    if not args.auto_pitch_warmup >= 0 or not args.auto_pitch_slew >= 0:
        sys.exit("infer_streaming.py: --auto-pitch-warmup and --auto-pitch-slew must be >= 0")
    slew = args.auto_pitch_slew * chunk / 24000 if args.auto_pitch_slew > 0 else float("inf")      # semitones per block
    return dict(new_frames=chunk // 480, window_frames=window, min_voiced=max(1, int(round(args.auto_pitch_warmup * FRAMES_PER_SECOND))), slew=slew)


def gate_sub_frames(ms):
    """milliseconds -> whole 10 ms sub-frames, rounded to the nearest"""
    return int(round(ms * 24.0 / GATE_SUB_FRAME))


def check_gate(args, block=None):
    """--gate and its six companions against each other and the stream's geometry, before anything is loaded: sys.exit with a message, or the
    StreamGate keywords (None without --gate).  `block`: the model's block length when it is not -c (--resample)"""
    extra = [f"--gate-{k}" for k in ("hysteresis", "range", "hold", "attack", "release", "lookahead") if getattr(args, f"gate_{k}") is not None]
    if args.gate is None:
        if extra:
            sys.exit(f"infer_streaming.py: {' '.join(extra)} without --gate DB: there is no gate to set")
        return None
    chunk = args.chunk if block is None else block
    hyst = 6.0 if args.gate_hysteresis is None else args.gate_hysteresis
    rng = -math.inf if args.gate_range is None else args.gate_range
    if math.isnan(args.gate):
        sys.exit("infer_streaming.py: --gate: a threshold in dB (--gate=-inf: always open)")
    if not (hyst >= 0 and math.isfinite(hyst)):
        sys.exit(f"infer_streaming.py: --gate-hysteresis {hyst}: a finite number of dB >= 0")
    if not rng <= 0:
        sys.exit(f"infer_streaming.py: --gate-range {rng}: a gain in dB <= 0 (-inf: silence)")
    ms = {k: (GATE_MS[k] if getattr(args, f"gate_{k}") is None else getattr(args, f"gate_{k}")) for k in GATE_MS}
    for k, v in ms.items():
        if not (v >= 0 and math.isfinite(v)):
            sys.exit(f"infer_streaming.py: --gate-{k} {v}: a finite number of milliseconds >= 0")
    if chunk <= 0 or chunk % GATE_SUB_FRAME:
        sys.exit(f"infer_streaming.py: --gate: blocks of {chunk} samples at 24 kHz are not whole {GATE_SUB_FRAME}-sample (10 ms) sub-frames")
    n = {k: gate_sub_frames(v) for k, v in ms.items()}
    n["attack"], n["release"] = max(1, n["attack"]), max(1, n["release"])      # a fade takes at least one sub-frame
    try:
        stream_gate_geometry(chunk, GATE_SUB_FRAME, n["lookahead"], n["hold"], n["attack"], n["release"])
        _, pad = check_window(chunk, args.extra, args.crossfade, args.sola_search, args.lookahead, bool(args.auto_pitch))
        check_gate_lookahead(n["lookahead"] * GATE_SUB_FRAME, args.crossfade, args.lookahead, pad)
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --gate: {e}")
    return dict(threshold_db=args.gate, hysteresis_db=hyst, range_db=rng, sub_frame=GATE_SUB_FRAME, hold_size=n["hold"] * GATE_SUB_FRAME,
                attack_size=n["attack"] * GATE_SUB_FRAME, release_size=n["release"] * GATE_SUB_FRAME, lookahead_size=n["lookahead"] * GATE_SUB_FRAME)


def check_denoise(args, block=None):
    """--denoise and its five companions against each other and the block, before anything is loaded: sys.exit with a message, or the
    StreamDenoise keywords (None without --denoise).  `block`: the model's block length when it is not -c (--resample)"""
    flags = dict(hop="hop", strength="strength", adapt="adapt_s", smooth="smooth_ms", warmup="warmup_ms")
    extra = [f"--denoise-{k}" for k in flags if getattr(args, f"denoise_{k}") is not None]
    if args.denoise is None:
        if extra:
            sys.exit(f"infer_streaming.py: {' '.join(extra)} without --denoise DB: there is no suppressor to set")
        return None
    chunk = args.chunk if block is None else block
    if math.isnan(args.denoise):
        sys.exit("infer_streaming.py: --denoise: a reduction in dB (0: the delayed input)")
    kw = {name: (DENOISE_DEFAULTS[name] if getattr(args, f"denoise_{k}") is None else getattr(args, f"denoise_{k}")) for k, name in flags.items()}
    for k, name in flags.items():
        if not (kw[name] >= 0 and math.isfinite(kw[name])):
            sys.exit(f"infer_streaming.py: --denoise-{k} {kw[name]}: a finite number >= 0")
    try:
        stream_denoise_geometry(chunk, kw["hop"])
        denoise_constants(clamp=2.0, **kw)
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --denoise: {e}")
    return dict(reduction_db=args.denoise, **kw)


def check_loudness(args, block=None):
    """--loudness and its four companions against each other and the block, before anything is loaded: sys.exit with a message, or the
    StreamLoudness keywords (None without --loudness).  `block`: the model's block length when it is not -c (--resample)"""
    extra = [f"--loudness-{k}" for k in LOUDNESS_DEFAULTS if getattr(args, f"loudness_{k}") is not None]
    if args.loudness is None:
        if extra:
            sys.exit(f"infer_streaming.py: {' '.join(extra)} without --loudness E: there is no stage to set")
        return None
    if not 0.0 <= args.loudness <= 1.0:      # (NaN fails both)
        sys.exit("infer_streaming.py: --loudness: a share in 0 .. 1")
    v = {k: (d if getattr(args, f"loudness_{k}") is None else getattr(args, f"loudness_{k}")) for k, d in LOUDNESS_DEFAULTS.items()}
    window = v["window"] * 24.0 / GATE_SUB_FRAME
    if not math.isfinite(window) or window != int(window) or int(window) % 2 != 1:
        sys.exit(f"infer_streaming.py: --loudness-window {v['window']:g}: an odd number of {GATE_SUB_FRAME / 24.0:g} ms sub-frames")
    chunk = args.chunk if block is None else block
    try:
        loudness_geometry(chunk, GATE_SUB_FRAME, (int(window) - 1) // 2, stream_block=True)
        loudness_levels(v["floor"], v["boost"], v["cut"], "--loudness")
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --loudness: {e}")
    return dict(share=args.loudness, sub_frame=GATE_SUB_FRAME, smooth=(int(window) - 1) // 2, floor_db=v["floor"], boost_db=v["boost"], cut_db=v["cut"])


def check_limit(args, block=None):
    """--limit and --limit-release against each other, -og and the block, before anything is loaded: sys.exit with a message, or the
    StreamLimiter keywords (None without --limit) - -og travels in them as drive_db, and the door then gets an output gain of 0.
    `block`: the model's block length when it is not -c (--resample)"""
    if args.limit is None:
        if args.limit_release is not None:
            sys.exit("infer_streaming.py: --limit-release without --limit [DB]: there is no stage to set")
        return None
    if not args.limit <= DOOR_CEILING_DB or args.limit < -600.0:      # (NaN fails the first)
        sys.exit(f"infer_streaming.py: --limit: a ceiling in dBFS of at most {DOOR_CEILING_DB:g} (above 32767 / 32768 the int16 conversion wraps)")
    ms = LIMIT_RELEASE_MS if args.limit_release is None else args.limit_release
    release = ms * 24.0 / LIMIT_SUB_FRAME
    if not math.isfinite(release) or release != int(release):
        sys.exit(f"infer_streaming.py: --limit-release {ms:g}: a whole number of {LIMIT_SUB_FRAME / 24.0:g} ms sub-frames")
    try:
        limiter_geometry(args.chunk if block is None else block, LIMIT_SUB_FRAME, int(release), stream_block=True)
        drive = limiter_drive(args.output_gain, "-og")
    except ValueError as e:
        sys.exit(f"infer_streaming.py: --limit: {e}")
    return dict(ceiling_db=args.limit, sub_frame=LIMIT_SUB_FRAME, release_size=int(release) * LIMIT_SUB_FRAME, drive_db=drive)


def main(argv=None):
    args = build_parser().parse_args(argv)
    block = check_resample(args)
    track_kw = check_auto_pitch(args, block)
    check_geometry(args, block)
    gate_kw = check_gate(args, block)
    denoise_kw = check_denoise(args, block)
    loudness_kw = check_loudness(args, block)
    limit_kw = check_limit(args, block)
    device = torch.device(args.device)
    if device.type != "cuda":
        sys.exit("infer_streaming.py: this build runs on an AMD GPU only; pass -d cuda")
    gen = load_generator(args.encoder_path, args.decoder_path, device)
    S = max(1, args.streams)
    if args.auto_pitch_from is not None and args.blend is not None:
        sys.exit("infer_streaming.py: --auto-pitch-from with --blend: a blend has no register of its own; use -p")
    tgt = load_target(gen, args, device)      # --blend (every stream takes the same mix), -idx or -t: as infer.py loads them
    pitch_shift = args.pitch_shift
    if args.auto_pitch_from is not None:      # one measurement, one host read, before the session starts
        reg = getattr(tgt, "pitch_register", None)
        if reg is None:
            sys.exit(f"infer_streaming.py: --auto-pitch-from: no pitch register beside {args.index} (extract_index.py writes <index>.f0.pt)")
        wf, sr = audio_io.load(args.auto_pitch_from)
        wf = gen.engine(device).resample(wf.to(device), sr, 24000)
        own = pitch_register(gen.encode(wf.mean(dim=0, keepdim=True))[1])
        if int(own.voiced[0]) == 0:
            sys.exit(f"infer_streaming.py: --auto-pitch-from: no voiced frame in {args.auto_pitch_from}")
        auto = semitones_between(float(own.median_hz[0]), float(reg.median_hz[0]))
        pitch_shift += auto
        print(f"Pitch register {float(own.median_hz[0]):.1f} Hz -> {float(reg.median_hz[0]):.1f} Hz: {auto:+.2f} semitones, session shift {pitch_shift:+.2f}")
    track = None
    if track_kw is not None:
        if getattr(tgt, "pitch_register", None) is None:
            sys.exit(f"infer_streaming.py: --auto-pitch: no pitch register beside {args.index} (extract_index.py writes <index>.f0.pt)")
        track = PitchTrack(S, lag_frames=args.lookahead // 480, device=device, **track_kw)      # the frames of the block about to be played (last_dilay_size)
    # the int16 conversions and gains belong to the door; without --resample it stands between equal rates - the samples are taken for
    # 24 kHz whatever -sr says, as in the reference - and is those conversions alone
    rate = args.sample_rate if block is not None else 24000
    # (with --limit -og is the limiter's drive, in front of it: a gain behind the limiter would lift its ceiling)
    door = StreamDoor(S, rate, rate, block if block is not None else args.chunk, args.input_gain, args.output_gain if limit_kw is None else 0.0, device=device)
    if block is not None:
        print(f"Resampling {rate} Hz <-> 24000 Hz on the device: {args.chunk}-sample blocks are {block} at the model's rate; "
              f"the two filters add {door.latency_seconds * 1e3:.2f} ms of latency")
    alpha_kw = alpha_keywords(args, "infer_streaming.py")      # {} without --alpha / --protect: the stream is then built as it has always been
    alpha_kw.update(match_weight_keywords(args, "infer_streaming.py"))      # likewise -k / --match-width
    alpha_kw.update(continuity_keywords(args, "infer_streaming.py", alpha_kw))      # likewise --continuity
    gate = None
    if gate_kw is not None:
        gate = StreamGate(S, door.block_size, device=device, **gate_kw)
        to_ms = 1000.0 / 24000
        print(f"Noise gate at {gate_kw['threshold_db']:g} dB (hysteresis {gate.hysteresis_db:g} dB, range {gate.range_db:g} dB): hold {gate.hold_size * to_ms:g} ms, "
              f"attack {gate.attack_size * to_ms:g} ms, release {gate.release_size * to_ms:g} ms, look-ahead {gate.lookahead_size * to_ms:g} ms "
              f"in {GATE_SUB_FRAME * to_ms:g} ms sub-frames")
    denoise = None
    if denoise_kw is not None:
        denoise = StreamDenoise(S, door.block_size, device=device, **denoise_kw)
        print(f"Noise suppressor: up to {denoise_kw['reduction_db']:g} dB per bin (strength {denoise.strength:g}, smoothing {denoise.smooth_ms:g} ms, adaptation "
              f"{denoise.adapt_s:g} s, warm-up {denoise.warmup_ms:g} ms) in 640-sample frames at a hop of {denoise.hop}: "
              f"{denoise.delay_size / 24000 * 1e3:.1f} ms of delay")
    if loudness_kw is not None:      # (absent: the stream is built as it has always been)
        alpha_kw["loudness"] = stage = StreamLoudness(S, door.block_size, device=device, **loudness_kw)
        print(f"Following {loudness_kw['share']:g} of the speaker's loudness envelope: {stage.window * GATE_SUB_FRAME / 24:g} ms window, floor {stage.floor_db:g} dB, "
              f"at most +{stage.boost_db:g} / -{stage.cut_db:g} dB")
    if limit_kw is not None:      # (absent: the stream is built as it has always been)
        alpha_kw["limiter"] = stage = StreamLimiter(S, door.block_size, device=device, **limit_kw)
        print(f"Peak limiter at {limit_kw['ceiling_db']:g} dBFS: drive {stage.drive_db:g} dB (-og), look-ahead and attack {stage.sub_frame / 24:g} ms, release "
              f"{stage.release_size / 24:g} ms")
    carry_kw = f0_carry_keywords(args, "infer_streaming.py")
    if carry_kw and door.block_size % 480:
        sys.exit(f"infer_streaming.py: --f0-carry: the block of {door.block_size} samples at 24 kHz is not a whole number of 480-sample frames")
    alpha_kw.update(carry_kw)
    tune_kw = tune_keywords(args, "infer_streaming.py")
    if tune_kw and door.block_size % 480:
        sys.exit(f"infer_streaming.py: --tune: the block of {door.block_size} samples at 24 kHz is not a whole number of 480-sample frames")
    alpha_kw.update(tune_kw)
    stream = BatchedStreamInfer(gen, n_streams=S, pitch_shift=pitch_shift, block_size=door.block_size, device=device, extra_size=args.extra,
                                f0_estimation=f0_keywords(args, "infer_streaming.py"), door=door, auto_pitch=True if track is not None else None, pitch_track=track,
                                crossfade_size=args.crossfade, sola_search_size=args.sola_search, last_delay_size=args.lookahead, gate=gate, denoise=denoise, **alpha_kw)
    lo, hi = stream.latency_seconds
    delay = f" + the suppressor's {denoise.delay_size}" if denoise is not None else ""
    if limit_kw is not None:
        delay += f" + the limiter's {stage.delay_size} (1 ms)"
    print(f"Latency {lo * 1e3:.1f} to {hi * 1e3:.1f} ms (cross-fade {args.crossfade} + look-ahead {args.lookahead} + lag 0 .. {args.sola_search}{delay} samples at 24 kHz"
          f"{', and the resampling filters' if block is not None else ''}) plus the {door.block_size / 24000 * 1e3:.0f} ms block")
    stream.target = tgt
    stream.init_buffer()

    def process(chunk_i16):
        """One pass of the reference's loop body (infer_streaming.py:84-94) for S streams: / 32768 and gain, the block, gain and * 32768 to
        int16 - with --resample also both resamplers -, all on the GPU"""
        pcm = torch.from_numpy(np.ascontiguousarray(chunk_i16)).to(device)
        return stream.audio_callback_pcm(pcm.expand(S, -1) if pcm.dim() == 1 else pcm).cpu().numpy()

    if args.input_wav is None:
        try:
            import pyaudio
        except ImportError:
            sys.exit("pyaudio is not installed: pass --input-wav / --output-wav for file-driven streaming")
        audio = pyaudio.PyAudio()
        sin = audio.open(format=pyaudio.paInt16, rate=args.sample_rate, channels=1, input_device_index=args.input, input=True)
        sout = audio.open(format=pyaudio.paInt16, rate=args.sample_rate, channels=1, output_device_index=args.output, output=True)
        sloop = audio.open(format=pyaudio.paInt16, rate=args.sample_rate, channels=1, output_device_index=args.loopback, output=True) if args.loopback != -1 else None
        print("Converting voice, Ctrl+C to stop conversion")
        while True:
            chunk = np.frombuffer(sin.read(args.chunk), dtype=np.int16)
            out = process(chunk)[0].tobytes()
            sout.write(out)
            if sloop is not None:
                sloop.write(out)

    blocks = int16_blocks_from_wav(args.input_wav, args.sample_rate, args.chunk, gen.engine(device))
    outs, lat = [], []
    ended_open = torch.zeros(S, dtype=torch.int64, device=device) if gate is not None else None
    for blk in blocks:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        o = process(blk)
        lat.append(time.perf_counter() - t0)      # includes the device -> host copy of the block, like the reference loop
        outs.append(o[0])
        if gate is not None:
            ended_open += gate.open      # counted on the device, read once at the end
    if args.output_wav:
        pcm = np.concatenate(outs).astype(np.float32) / 32768
        audio_io.save(args.output_wav, torch.from_numpy(pcm)[None], args.sample_rate)
    if track is not None:
        reg = track.register()
        for s_, (hz, n, sh) in enumerate(zip(reg.median_hz.tolist(), reg.voiced.tolist(), stream.last_pitch_shift.tolist())):
            print(f"stream {s_}: register {hz:.1f} Hz over {n} voiced frames, shift {sh:+.2f} semitones")
    if gate is not None and blocks:
        for s_, n_open in enumerate(ended_open.tolist()):
            print(f"stream {s_}: gate open at the end of {n_open} of {len(blocks)} blocks ({100.0 * n_open / len(blocks):.0f} %)")
    if denoise is not None and blocks:
        for s_, db in enumerate(denoise.noise_db.tolist()):
            print(f"stream {s_}: noise estimate {db:.1f} dB re full scale")
    if len(lat) > 3:
        l = np.sort(np.array(lat[3:])) * 1e3
        budget = args.chunk / args.sample_rate * 1e3
        print(f"{S} stream(s), {len(lat)} blocks: p50 {l[len(l) // 2]:.2f} ms, p95 {l[int(len(l) * 0.95)]:.2f} ms per block (real-time budget {budget:.0f} ms)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
