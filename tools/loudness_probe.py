"""What does the loudness envelope match cost, and does a stream without it cost what it did?  (Not part of the bench; run on the GPU box.)

Fresh processes that take turns (tools/alpha_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, a 1000-vector index, use_graph=True), 220 blocks
            after 20 warm-up blocks, p50 / p95 of the block latency: this tree's library without the stage (`default`), with
            `--parent-lib PATH` - a build of the parent commit - that library too (`parent`), and this tree's with
            StreamLoudness(share=1) (`loudness`: the stage's launch inside the same captured graph)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
and, in one more process, by hipEvents over 200 launches issued from Python:
  the stream launch alone (tvc_stream_loudness_f32, 1920-sample blocks in 240-sample sub-frames, 13 440-sample windows) at S = 32 and 4 096
  the offline launch (tvc_loudness_match_f32) on the 64 x 4 s batch and on one five-minute row, into a tensor of its own and in place
  (one workgroup per row)
The one condition: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread,
README) - a stream or a call without the stage launches what it launched before.  Everything else is recorded, not gated.
Writes profiles/loudness_probe.json and prints it as one JSON line."""
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
NEW_ENTRIES = ("tvc_loudness_geometry", "tvc_loudness_geometry_message", "tvc_stream_loudness_geometry", "tvc_stream_loudness_geometry_message",
               "tvc_loudness_match_f32", "tvc_stream_loudness_f32")


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
    if mode == "loudness":
        from tinyvc_amd.module.infer import StreamLoudness
        kw["loudness"] = StreamLoudness(S, 1920, share=1.0, device=dev)
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True, **kw)
    st.init_buffer()
    waves = torch.stack([synth.synth_wave(1, BLOCKS * 1920, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(S) % 4].to(dev).view(S, BLOCKS, 1920).clone()
    if mode == "loudness":
        waves[1::2] *= 0.05      # every other speaker murmurs
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
    if mode == "loudness":
        res["gain_db_at_the_end"] = [round(float(v), 2) for v in (st.loudness.gain_db[0::2].mean(), st.loudness.gain_db[1::2].mean())]
        assert st.loudness.frames.tolist() == [BLOCKS * 8] * S
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
    import torch
    from tinyvc_amd.engine import default_engine
    from tinyvc_amd.module.infer import StreamLoudness
    dev = torch.device("cuda", 0)
    eng = default_engine(dev)
    res = {}
    for S in (32, 4096):
        stage = StreamLoudness(S, 1920, share=1.0, device=dev)
        x = torch.randn(S, 13440, device=dev) * 0.1
        y = torch.randn(S, 1920, device=dev) * 0.3
        out = torch.empty_like(y)
        shift = torch.randint(0, 1921, (S,), dtype=torch.int32, device=dev)
        res[f"kernel_s{S}_ms"] = _events_ms(lambda: eng.stream_loudness(x, y, shift, stage, 3840, out=out))
    B, L = 64, 4 * 24000
    x, y = torch.randn(B, L, device=dev) * 0.1, torch.randn(B, L, device=dev) * 0.3
    share = torch.ones(B, device=dev)
    out = torch.empty_like(y)
    res["offline_64x4s_ms"] = _events_ms(lambda: eng.loudness_match(x, y, share, out=out))
    res["offline_64x4s_in_place_ms"] = _events_ms(lambda: eng.loudness_match(x, y, share, out=y))
    res["offline_64x4s_bytes"] = 3 * B * L * 4      # x and y read, out written (y's second read is served by the caches)
    L = 300 * 24000      # one five-minute row: 469 tiles, in place on one workgroup
    x, y = torch.randn(1, L, device=dev) * 0.1, torch.randn(1, L, device=dev) * 0.3
    out = torch.empty_like(y)
    res["offline_1x300s_ms"] = _events_ms(lambda: eng.loudness_match(x, y, share[:1], out=out), 50)
    res["offline_1x300s_in_place_ms"] = _events_ms(lambda: eng.loudness_match(x, y, share[:1], out=y), 20)
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"loudness_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child), ("--kernel-child", kernel_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "loudness"]
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[loudness probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[loudness probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["loudness_over_default_ms"] = round(res["loudness_p50_ms"] - res["default_p50_ms"], 4)
    res["loudness_gain_db_at_the_end"] = runs["loudness"][-1]["gain_db_at_the_end"]
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    res.update(run_child("--kernel-child", "default", parent_lib))
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "loudness_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("loudness_probe: a stream or a bench step without the stage is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
