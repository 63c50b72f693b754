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

`--streams S` feeds S copies of the input as S concurrent streams through one BatchedStreamInfer
(one batched convert + one SOLA launch per block) and reports the p50 / p95 block latency against the
real-time budget (chunk / 24 kHz = 80 ms for the default 1920-sample chunk).
"""
import argparse
import sys
import time

import numpy as np
import torch

from tinyvc_amd import audio_io
from infer import load_generator, load_target
from tinyvc_amd.module.infer import BatchedStreamInfer
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack, add_blend_argument, pitch_register, semitones_between

FRAMES_PER_SECOND = 50      # 24 kHz / 480 samples


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
    p.add_argument("-c", "--chunk", default=1920, type=int)
    p.add_argument("-e", "--extra", default=3840, type=int)
    p.add_argument("-d", "--device", default="cuda")
    p.add_argument("-sr", "--sample-rate", default=24000, type=int)
    p.add_argument("-ig", "--input-gain", default=0, type=float)
    p.add_argument("-og", "--output-gain", default=0, type=float)
    p.add_argument("-f0-est", "--f0-estimation", default="default", choices=["default", "fcpe", "dio", "harvest"])
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


def check_auto_pitch(args):
    """--auto-pitch against the other flags, before anything is loaded: sys.exit with a message, or the PitchTrack keywords (None without
    the flag)"""
    if not args.auto_pitch:
        return None
    if args.auto_pitch_from is not None:
        sys.exit("infer_streaming.py: --auto-pitch with --auto-pitch-from: the live tracker needs no calibration recording; pick one")
    if args.blend is not None:
        sys.exit("infer_streaming.py: --auto-pitch with --blend: a blend has no register of its own; use -p")
    if args.chunk <= 0 or args.chunk % 480:
        sys.exit(f"infer_streaming.py: --auto-pitch: -c {args.chunk} is not a whole number of 480-sample frames")
    if args.chunk // 480 > 256:
        sys.exit(f"infer_streaming.py: --auto-pitch: -c {args.chunk} is more than 256 frames per block")
    window = int(round(args.auto_pitch_window * FRAMES_PER_SECOND))
    if not 1 <= window <= 8192:
        sys.exit("infer_streaming.py: --auto-pitch-window: between 0.02 and 163.84 seconds")
    if not args.auto_pitch_warmup >= 0 or not args.auto_pitch_slew >= 0:
        sys.exit("infer_streaming.py: --auto-pitch-warmup and --auto-pitch-slew must be >= 0")
    slew = args.auto_pitch_slew * args.chunk / 24000 if args.auto_pitch_slew > 0 else float("inf")      # semitones per block
    return dict(new_frames=args.chunk // 480, window_frames=window, min_voiced=max(1, int(round(args.auto_pitch_warmup * FRAMES_PER_SECOND))), slew=slew)


def main(argv=None):
    args = build_parser().parse_args(argv)
    track_kw = check_auto_pitch(args)
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
        track = PitchTrack(S, lag_frames=3840 // 480, device=device, **track_kw)      # the frames of the block about to be played (last_dilay_size)
    stream = BatchedStreamInfer(gen, n_streams=S, pitch_shift=pitch_shift, block_size=args.chunk, device=device,
                                extra_size=args.extra, f0_estimation=args.f0_estimation, auto_pitch=True if track is not None else None, pitch_track=track)
    stream.target = tgt
    stream.init_buffer()

    def process(chunk_i16):
        """One pass of the reference's loop body (infer_streaming.py:84-94) for S streams."""
        eng = gen.engine(device)
        x = eng.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(chunk_i16)).to(device), args.input_gain)      # / 32768, gain: on the GPU
        y = stream.audio_callback(x.expand(S, -1) if x.dim() == 1 else x)
        return eng.f32_to_pcm16(y, args.output_gain).cpu().numpy()                                                # gain, * 32768, int16: on the GPU

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
    for blk in blocks:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        o = process(blk)
        lat.append(time.perf_counter() - t0)      # includes the device -> host copy of the block, like the reference loop
        outs.append(o[0])
    if args.output_wav:
        pcm = np.concatenate(outs).astype(np.float32) / 32768
        audio_io.save(args.output_wav, torch.from_numpy(pcm)[None], args.sample_rate)
    if track is not None:
        reg = track.register()
        for s_, (hz, n, sh) in enumerate(zip(reg.median_hz.tolist(), reg.voiced.tolist(), stream.last_pitch_shift.tolist())):
            print(f"stream {s_}: register {hz:.1f} Hz over {n} voiced frames, shift {sh:+.2f} semitones")
    if len(lat) > 3:
        l = np.sort(np.array(lat[3:])) * 1e3
        budget = args.chunk / args.sample_rate * 1e3
        print(f"{S} stream(s), {len(lat)} blocks: p50 {l[len(l) // 2]:.2f} ms, p95 {l[int(len(l) * 0.95)]:.2f} ms per block (real-time budget {budget:.0f} ms)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
