"""What does the look-ahead peak limiter cost, and does a stream without it cost what it did?  (Not part of the bench; run on the GPU box.)

Fresh processes that take turns (tools/alpha_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, a 1000-vector index, use_graph=True), 220 blocks
            after 20 warm-up blocks, p50 / p95 of the block latency: this tree's library without the stage (`default`), with
            `--parent-lib PATH` - a build of the parent commit - that library too (`parent`), and this tree's with
            StreamLimiter(ceiling_db=-12) (`limiter`: the stage's launch inside the same captured graph)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
and, in one more process, by hipEvents over 200 launches issued from Python:
  the stream launch alone (tvc_stream_limit_f32, 1920-sample blocks in 24-sample sub-frames, release 100) at S = 32 and 4 096
  the offline launch (tvc_limit_f32) on the 64 x 4 s batch (release 100) and on one five-minute row at release 100 and 4096
The one condition: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread,
README) - a stream or a call without the stage launches what it launched before.  Everything else is recorded, not gated.
Writes profiles/limiter_probe.json and prints it as one JSON line."""
import io
import json
import os
import subprocess
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, BLOCKS, WARM = 32, 240, 20
NEW_ENTRIES = ("tvc_limiter_geometry", "tvc_limiter_geometry_message", "tvc_stream_limiter_geometry", "tvc_stream_limiter_geometry_message", "tvc_limit_f32",
               "tvc_stream_limit_f32")


def as_parent():
    """the parent commit's library has every entry but the new ones, which a stream or a call without the stage never reaches"""
    from tinyvc_amd import _lib
    for name in NEW_ENTRIES:
        _lib.SIGNATURES.pop(name, None)


def stream_child(mode):
    """one stream run in this process -> {"p50_ms", "p95_ms"} as a JSON line"""
    import numpy as np
    import torch
    if mode == "parent":
        as_parent()
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.infer import BatchedStreamInfer
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    S = STREAMS
    kw = {}
    if mode == "limiter":
        from tinyvc_amd.module.infer import StreamLimiter
        kw["limiter"] = StreamLimiter(S, 1920, ceiling_db=-12.0, device=dev)
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True, **kw)
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
    assert out.shape == (S, 1920) and bool(out.abs().max() > 0)
    res = {}
    if mode == "limiter":
        res["reduction_db_at_the_end"] = round(float(st.limiter.reduction_db.mean()), 2)
        res["output_peak"] = round(float(out.abs().max()), 6)
        assert float(out.abs().max()) <= float(st.limiter.ceiling[0])
    l = np.sort(np.array(lat[WARM:])) * 1e3
    res.update({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])})
    print(json.dumps(res))


def bench_child(mode):
    """bench.py's own timed steps in this process -> {"value"} as a JSON line"""
    if mode == "parent":
        as_parent()
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-stream", "--no-parity"]
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    res = json.loads(buf.getvalue().strip().splitlines()[-1])
    print(json.dumps({"value": res["value"]}))


def _events_ms(fn, launches=200):
    import torch
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def kernel_child(_mode):
    """the two launches alone: milliseconds per launch by hipEvents"""
    import types

    import torch
    from tinyvc_amd.engine import default_engine
    from tinyvc_amd.module.infer import StreamLimiter
    dev = torch.device("cuda", 0)
    eng = default_engine(dev)
    res = {}
    for S in (32, 4096):
        stage = StreamLimiter(S, 1920, ceiling_db=-12.0, device=dev)
        y = torch.randn(S, 1920, device=dev) * 0.3
        res[f"kernel_s{S}_ms"] = _events_ms(lambda: eng.stream_limit(y, stage))
    B, L = 64, 4 * 24000
    y = torch.randn(B, L, device=dev) * 0.3
    ceiling = torch.full((B,), 0.25, device=dev)
    res["offline_64x4s_ms"] = _events_ms(lambda: eng.limit(y, ceiling))
    res["offline_64x4s_bytes"] = 2 * B * L * 4      # y read, out written (the halo and y's second read are served by the caches)
    res["offline_64x4s_tb_per_s"] = res["offline_64x4s_bytes"] / (res["offline_64x4s_ms"] * 1e-3) / 1e12
    L = 300 * 24000      # one five-minute row: 300 000 sub-frames
    y = torch.randn(1, L, device=dev) * 0.3
    for R in (100, 4096):
        settings = types.SimpleNamespace(sub_frame=24, release=R, drive_db=0.0)
        res[f"offline_1x300s_release{R}_ms"] = _events_ms(lambda: eng.limit(y, ceiling[:1], settings=settings), 50)
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"limiter_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child), ("--kernel-child", kernel_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "limiter"]
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[limiter probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[limiter probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["limiter_over_default_ms"] = round(res["limiter_p50_ms"] - res["default_p50_ms"], 4)
    res["limiter_reduction_db_at_the_end"] = runs["limiter"][-1]["reduction_db_at_the_end"]
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    res.update(run_child("--kernel-child", "default", parent_lib))
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "limiter_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("limiter_probe: a stream or a bench step without the stage is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
