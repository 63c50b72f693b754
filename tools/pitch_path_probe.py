"""What does the pitch path cost, and does a stream without it cost what it did?  (Not part of the bench; run on the GPU box.)

Fresh processes that take turns (tools/alpha_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, a 1000-vector index, use_graph=True), 220 blocks
            after 20 warm-up blocks, p50 / p95 of the block latency: this tree's library without the path (`default`), with
            `--parent-lib PATH` - a build of the parent commit - that library too (`parent`), and this tree's with
            f0_estimation='viterbi' (`path`: the path kernel inside the same captured graph, each 28-frame window decoded afresh)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
and, in one more process, by hipEvents:
  the 64 x 4 s batch (Generator.convert, one index per row) with and without the path, 20 calls each
  the stage launch alone (tvc_pitch_path_f32, the default settings, Gaussian logits) at (64 rows x 200 frames), (32 x 28), (4 096 x 28)
  and (1 x 15 000) - the last is ONE workgroup walking 15 000 dependent frames and then back
The one condition: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread,
README) - a stream or a call without the path launches what it launched before.  Everything else is recorded, not gated.
Writes profiles/pitch_path_probe.json and prints it as one JSON line."""
import ctypes
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
NEW_ENTRIES = ("tvc_workspace_bytes_pitch_path", "tvc_pitch_path_f32", "tvc_workspace_bytes_path", "tvc_convert_path_f32", "tvc_workspace_bytes_ragged_path",
               "tvc_convert_ragged_path_f32")
STAGE_SHAPES = ((64, 200), (32, 28), (4096, 28), (1, 15000))


def as_parent():
    """the parent commit's library has every entry but the new ones, which a stream or a call without the path never reaches"""
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
    kw = {"f0_estimation": "viterbi"} if mode == "path" else {}
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


def _events_ms(fn, launches, warm=3):
    import torch
    for _ in range(warm):
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
    """the batch with and without the path, and the stage launch alone: milliseconds per call by hipEvents"""
    import torch
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    res = {}
    B, L = 64, 4 * 24000
    wf = synth.synth_wave(4, L, seed=300)[torch.arange(B) % 4].to(dev).contiguous()
    tgt = [synth.synth_index(1000, seed=2).to(dev)] * B
    angle = synth.synth_angle(1, L // 480, 5).to(dev).expand(B, -1, -1).contiguous()
    res["batch_64x4s_ms"] = _events_ms(lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle), 20)
    res["batch_64x4s_path_ms"] = _events_ms(lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle, f0_estimation="viterbi"), 20)
    res["batch_64x4s_path_over_plain"] = res["batch_64x4s_path_ms"] / res["batch_64x4s_ms"] - 1.0
    settings = PitchPath().settings()
    for rows, T in STAGE_SHAPES:      # the entry itself on buffers made once: Engine.pitch_path would add four allocations and their memsets
        x = torch.randn(rows, 512, T, device=dev)
        I64 = ctypes.c_int64 * rows
        start, count = I64(*(b * T for b in range(rows))), I64(*([T] * rows))
        f0, path = torch.empty(rows, T, device=dev), torch.empty(rows, T, dtype=torch.int32, device=dev)
        p, n = eng._query_ws("tvc_workspace_bytes_pitch_path", start, count, rows)

        def launch():
            eng._ok(eng.lib.tvc_pitch_path_f32(eng.ctx, eng._stream(), x.data_ptr(), start, count, rows, T, ctypes.byref(settings), 0.0, None, f0.data_ptr(),
                                               None, path.data_ptr(), None, p, n), "tvc_pitch_path_f32")
        res[f"stage_{rows}x{T}_ms"] = _events_ms(launch, 20 if rows * T < 100000 else 5, warm=2)
        del x
    res["stage_1x15000_us_per_frame"] = res["stage_1x15000_ms"] * 1e3 / 15000
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"pitch_path_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child), ("--kernel-child", kernel_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "path"]
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[pitch path probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[pitch path probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["path_over_default_ms"] = round(res["path_p50_ms"] - res["default_p50_ms"], 4)
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    res.update(run_child("--kernel-child", "default", parent_lib))
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "pitch_path_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("pitch_path_probe: a stream or a bench step without the path is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
