"""What does serving streams at the sound card's rate cost per block?  (Not part of the bench; run on the GPU box.)

BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, 13 440-sample buffers, a 1000-vector index, use_graph=True),
220 blocks after 20 warm-up blocks, p50 / p95 of the block latency:
  float              door-less BatchedStreamInfer.audio_callback on fp32 blocks, as it was: this tree's library, and - with `--parent-lib PATH`,
                     a build of the parent commit - that library too, each in fresh processes that take turns (tools/ab_latency.sh's scheme),
                     twice each
  door48k            BatchedStreamInfer(door=StreamDoor(S, 48000)).audio_callback_pcm: int16 at 48 kHz in, int16 at 48 kHz out, the two
                     door launches inside the same captured graph
and the door's launch alone (tvc_stream_resample, 48 kHz int16 -> 24 kHz fp32, 3840-sample blocks, hipEvent time over 200 launches) at
S = 32 and S = 4096.
Gate: the float p50 of this tree within 3 % of the parent library's (the pool's box-to-box spread, README): the door-less path launches
nothing new.  The door figure is recorded, not gated: there is no earlier number to hold it against.
Writes profiles/stream_door_probe.json and prints it as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, BLOCKS, WARM = 32, 240, 20
NEW_ENTRIES = ("tvc_stream_resample_geometry", "tvc_stream_resample_prepare", "tvc_stream_resample")


def child(mode):
    """one stream run in this process -> {"p50_ms", "p95_ms"} as a JSON line"""
    import numpy as np
    import torch
    from tinyvc_amd import _lib
    if mode == "parent":      # the parent commit's library has every entry but the new ones, which the door-less path never calls
        for name in NEW_ENTRIES:
            _lib.SIGNATURES.pop(name, None)
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    S = STREAMS
    door = StreamDoor(S, 48000, device=dev) if mode == "door48k" else None
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True,
                            door=door)
    st.init_buffer()
    chunk = door.chunk_in if door is not None else 1920
    waves = torch.stack([synth.synth_wave(1, BLOCKS * chunk, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(S) % 4].to(dev).view(S, BLOCKS, chunk)
    if door is not None:
        waves = (waves * 0.8 * 32767).to(torch.int16)
    call = st.audio_callback_pcm if door is not None else st.audio_callback
    lat = []
    for i in range(BLOCKS):
        blk = waves[:, i].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = call(blk)
        torch.cuda.synchronize(dev)
        lat.append(time.perf_counter() - t0)
    assert out.dtype == (torch.int16 if door is not None else torch.float32) and bool(out.to(torch.float32).abs().max() > 0)
    l = np.sort(np.array(lat[WARM:])) * 1e3
    print(json.dumps({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])}))


def kernel_ms(S, launches=200):
    """the door's launch alone: milliseconds per launch by hipEvents around `launches` of them"""
    import torch
    from tinyvc_amd.engine import default_engine
    dev = torch.device("cuda", 0)
    eng = default_engine(dev)
    n_out, hist, _ = eng.stream_resample_geometry(48000, 24000, 3840)
    pcm = torch.randint(-20000, 20000, (S, 3840), dtype=torch.int32, device=dev).to(torch.int16)
    state = torch.zeros(S, hist, device=dev)
    for _ in range(10):
        eng.stream_resample(pcm, state, 48000, 24000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(launches):
        eng.stream_resample(pcm, state, 48000, 24000)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / launches


def main():
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["float", "door48k"]
    runs = {m: [] for m in modes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            env = dict(os.environ)
            if m == "parent":
                env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
            if out.returncode != 0:
                sys.exit(f"stream_door_probe: the {m} run failed:\n{out.stdout}{out.stderr}")
            runs[m].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"[stream door probe] {m}: {runs[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["door48k_over_float_ms"] = round(res["door48k_p50_ms"] - res["float_p50_ms"], 4)
    if parent_lib:
        res["float_vs_parent"] = round(res["float_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["float_within_3_percent_of_parent"] = bool(abs(res["float_vs_parent"]) <= 0.03)
    for S in (32, 4096):
        res[f"kernel_48k_pcm16_in_s{S}_ms"] = round(kernel_ms(S), 5)
    with open(os.path.join(ROOT, "profiles", "stream_door_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["float_within_3_percent_of_parent"]:
        sys.exit("stream_door_probe: the door-less stream is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
