"""What does the match along a path (continuity) cost, and does a call without it cost what it did?  (Not part of the bench; run on the GPU box.)

Fresh processes that take turns (tools/alpha_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: a 1000-vector index, use_graph=True), 220 blocks after 20 warm-up
            blocks, p50 / p95 of the block latency: this tree's library without the feature (`default`), with `--parent-lib PATH` - a build of
            the parent commit - that library too (`parent`), and this tree's with k = 4, a width of 0.02 and c = 0.5 (`joined`)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
  batch     configs[1]'s 64 x 4 s batch against a 10 000-vector index through Generator.convert, with k = 4 / width 0.02 without and with
            c = 0.5: the median step of 20 after 3 warm-up steps, the two routes taking turns in one process
  stage     the stage call at that shape (64 x 768 x 200) by hipEvents over 100 calls: Engine.knn_match_weighted and Engine.knn_match_joined
            with the same k and width - the search is the same launches, so their difference is what the merge + affinity launch, the path
            launch and the joined form of the gather add
  path      the path launch alone, and the merge + affinity launch alone, at 32 x 28 columns (a set of streams' windows) and at 1 x 15 000
            (one long utterance: the path is one wavefront's serial walk) against a 1000-vector index: the library's own profile regions
            "knn.join_path" and "knn.join_affinity" (hipEvents around each launch, Engine.profile) over 50 calls; beside them the same
            joined-minus-weighted difference of the whole stage call
Gate: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread, README): a call
without the feature launches what it launched before.  Everything else is recorded, not gated.
Writes profiles/match_join_probe.json and prints it as one JSON line."""
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
K, WIDTH, C = 4, 0.02, 0.5
NEW_ENTRIES = ("tvc_knn_match_joined_f32", "tvc_joined_convert_f32", "tvc_joined_convert_ragged_f32", "tvc_workspace_bytes_joined",
               "tvc_workspace_bytes_ragged_joined", "tvc_workspace_bytes_match_joined")
STREAM_MODES = {"default": {}, "joined": dict(k=K, match_width=WIDTH, continuity=C)}


def as_parent():
    """the parent commit's library has every entry but the new ones"""
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
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True,
                            **STREAM_MODES.get(mode, {}))
    st.init_buffer()
    waves = torch.stack([synth.synth_wave(1, BLOCKS * 1920, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(S) % 4].to(dev).view(S, BLOCKS, 1920)
    lat = []
    for i in range(BLOCKS):
        blk = waves[:, i].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = st.audio_callback(blk)
        torch.cuda.synchronize(dev)
        lat.append(time.perf_counter() - t0)
    assert out.shape == (S, 1920) and bool(out.abs().max() > 0)
    l = np.sort(np.array(lat[WARM:])) * 1e3
    print(json.dumps({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])}))


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


def _events(torch, dev, fn, calls=100):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


def batch_child(_mode):
    """the 64 x 4 s batch without and with the path, and the stage call's weighted and joined forms by hipEvents at three shapes"""
    import torch
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_reference
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    B, L, N = 64, 4 * 24000, 10000
    wf = synth.synth_wave(B, L, seed=100).to(dev)
    tgt = synth.synth_index(N, seed=8).to(dev)
    angle = synth.synth_angle(B, L // 480, 3).to(dev)
    k = torch.full((B,), K, dtype=torch.int32, device=dev)
    width = torch.full((B,), WIDTH, device=dev)
    c = torch.full((B,), C, device=dev)
    routes = {"batch_weighted_ms": lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle, k=k, match_width=width),
              "batch_joined_ms": lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle, k=k, match_width=width, continuity=c)}
    ts = {n: [] for n in routes}
    for r in range(23):
        for n, fn in routes.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if r >= 3:
                ts[n].append((time.perf_counter() - t0) * 1e3)
    res = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
    blob, n = prepare_reference(tgt)
    src = torch.randn(B, 768, L // 480, device=dev)
    res["match_weighted_ms"] = _events(torch, dev, lambda: eng.knn_match_weighted(src, [blob] * B, [n] * B, k, width))
    res["match_joined_ms"] = _events(torch, dev, lambda: eng.knn_match_joined(src, [blob] * B, [n] * B, c, k, width))
    res["stage_join_adds_ms"] = res["match_joined_ms"] - res["match_weighted_ms"]
    small, ns = prepare_reference(synth.synth_index(1000, seed=2).to(dev))
    for name, (rows, T) in (("32x28", (32, 28)), ("1x15000", (1, 15000))):
        s = torch.randn(rows, 768, T, device=dev)
        kk, ww, cc = k[:rows].contiguous(), width[:rows].contiguous(), c[:rows].contiguous()
        weighted = _events(torch, dev, lambda: eng.knn_match_weighted(s, [small] * rows, [ns] * rows, kk, ww))
        joined = _events(torch, dev, lambda: eng.knn_match_joined(s, [small] * rows, [ns] * rows, cc, kk, ww))
        res[f"path_{name}_weighted_ms"], res[f"path_{name}_joined_ms"], res[f"path_{name}_adds_ms"] = weighted, joined, joined - weighted
        eng.profile(True)
        eng.profile_read()
        for _ in range(50):
            eng.knn_match_joined(s, [small] * rows, [ns] * rows, cc, kk, ww)
        regions = eng.profile_read()
        eng.profile(False)
        res[f"path_{name}_path_launch_ms"] = regions["knn.join_path"] / 50
        res[f"path_{name}_affinity_launch_ms"] = regions["knn.join_affinity"] / 50
    print(json.dumps({n: round(v, 5) for n, v in res.items()}))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"match_join_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child), ("--batch-child", batch_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + list(STREAM_MODES)
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[match join probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[match join probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True, "joined": {"k": K, "match_width": WIDTH, "continuity": C}}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["joined_over_default"] = round(res["joined_p50_ms"] / res["default_p50_ms"], 4)
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    res.update(run_child("--batch-child", "default", parent_lib))
    res["batch_joined_over_weighted"] = round(res["batch_joined_ms"] / res["batch_weighted_ms"], 4)
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "match_join_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("match_join_probe: a call without the feature is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
