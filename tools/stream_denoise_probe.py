"""What does a spectral suppressor in front of the window cost per block?  (Not part of the bench; run on the GPU box.)

BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, 13 440-sample buffers, a 1000-vector index, use_graph=True),
220 blocks after 20 warm-up blocks, p50 / p95 of the block latency:
  float              BatchedStreamInfer.audio_callback without a suppressor, as it was: this tree's library, and - with `--parent-lib PATH`, a
                     build of the parent commit - that library too, each in fresh processes that take turns, twice each
  denoise            BatchedStreamInfer(denoise=StreamDenoise(S, 1920)).audio_callback: the suppressor's launch inside the same captured graph
and the suppressor's launch alone (tvc_stream_denoise_f32, 1920-sample blocks at hop 160: 12 frames in two groups; hipEvent time over 200
launches) at S = 32 and S = 4096.
The one condition: the float p50 of this tree within 3 % of the parent library's (the pool's box-to-box spread, README) - the path without
a suppressor launches nothing new.  The suppressor's figures are recorded, not held against anything: there is no earlier number.
Writes profiles/stream_denoise_probe.json and prints it as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, BLOCKS, WARM = 32, 240, 20
NEW_ENTRIES = ("tvc_stream_denoise_geometry", "tvc_stream_denoise_geometry_message", "tvc_stream_denoise_f32")


def child(mode):
    """one stream run in this process -> {"p50_ms", "p95_ms"} as a JSON line"""
    import numpy as np
    import torch
    from tinyvc_amd import _lib
    if mode == "parent":      # the parent commit's library has every entry but the new ones, which the path without a suppressor never calls
        for name in NEW_ENTRIES:
            _lib.SIGNATURES.pop(name, None)
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDenoise
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    S = STREAMS
    dn = StreamDenoise(S, 1920, device=dev) if mode == "denoise" else None
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True,
                            denoise=dn)
    st.init_buffer()
    waves = torch.stack([synth.synth_wave(1, BLOCKS * 1920, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(S) % 4].to(dev).view(S, BLOCKS, 1920).clone()
    lat = []
    for i in range(BLOCKS):
        blk = waves[:, i].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = st.audio_callback(blk)
        torch.cuda.synchronize(dev)
        lat.append(time.perf_counter() - t0)
    assert out.dtype == torch.float32 and bool(out.abs().max() > 0)
    res = {}
    if dn is not None:
        assert min(dn.frames.tolist()) > 0, "the suppressor did not run"
        res["noise_db_stream0"] = round(float(dn.noise_db[0]), 2)
    l = np.sort(np.array(lat[WARM:])) * 1e3
    res.update({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])})
    print(json.dumps(res))


def kernel_ms(S, launches=200):
    """the suppressor's launch alone: milliseconds per launch by hipEvents around `launches` of them"""
    import torch
    from tinyvc_amd.engine import default_engine
    from tinyvc_amd.module.infer import StreamDenoise
    dev = torch.device("cuda", 0)
    eng = default_engine(dev)
    dn = StreamDenoise(S, 1920, device=dev)
    x = torch.randn(S, 1920, device=dev) * 0.1
    out = torch.empty_like(x)
    for _ in range(10):
        eng.stream_denoise(x, dn, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(launches):
        eng.stream_denoise(x, dn, out=out)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / launches


def main():
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["float", "denoise"]
    runs = {m: [] for m in modes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            env = dict(os.environ)
            if m == "parent":
                env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
            if out.returncode != 0:
                sys.exit(f"stream_denoise_probe: the {m} run failed:\n{out.stdout}{out.stderr}")
            runs[m].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"[stream denoise probe] {m}: {runs[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["denoise_over_float_ms"] = round(res["denoise_p50_ms"] - res["float_p50_ms"], 4)
    res["denoise_noise_db_stream0"] = runs["denoise"][-1]["noise_db_stream0"]
    if parent_lib:
        res["float_vs_parent"] = round(res["float_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["float_within_3_percent_of_parent"] = bool(abs(res["float_vs_parent"]) <= 0.03)
    for S in (32, 4096):
        res[f"kernel_s{S}_ms"] = round(kernel_ms(S), 5)
    with open(os.path.join(ROOT, "profiles", "stream_denoise_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["float_within_3_percent_of_parent"]:
        sys.exit("stream_denoise_probe: the stream without a suppressor is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
