"""What does carrying the pitch path's scores cost, and does a stream without the path cost what it did?  (Not part of the bench; run on the
GPU box.)

Fresh processes that take turns (tools/pitch_path_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, a 1000-vector index, use_graph=True), 220 blocks
            after 20 warm-up blocks, p50 / p95 of the block latency: this tree's library without the path (`default`), with
            `--parent-lib PATH` - a build of the parent commit - that library too (`parent`), this tree's with f0_estimation='viterbi'
            (`path`: every 28-frame window decoded afresh) and with f0_carry=True on top (`carry`: the carried variant of the path kernel in
            the same captured graph - one more barrier at frame 0, one 4-byte store per thread at frame 4)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
The one condition: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread,
README) - a stream or a call without the path launches what it launched before.  `carry` against `path` is recorded, not gated.
Writes profiles/pitch_carry_probe.json and prints it as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pitch_path_probe as base  # noqa: E402  (its bench child and constants are this probe's too)

STREAMS, BLOCKS, WARM = base.STREAMS, base.BLOCKS, base.WARM
NEW_ENTRIES = ("tvc_pitch_path_carry_f32", "tvc_convert_carry_f32")
STREAM_KW = {"parent": {}, "default": {}, "path": {"f0_estimation": "viterbi"}, "carry": {"f0_estimation": "viterbi", "f0_carry": True}}


def as_parent():
    """the parent commit's library has every entry but the new ones, which a stream or a call without the carry never reaches"""
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
                            **STREAM_KW[mode])
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
    if mode == "carry":      # the state did travel: every stream's scores are a carry (maximum exactly 0), not the zeros of a fresh path
        sc = st.pitch_carry.scores
        assert bool((sc.max(dim=1).values == 0).all()) and bool((sc != 0).any(dim=1).all())
    l = np.sort(np.array(lat[WARM:])) * 1e3
    print(json.dumps({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])}))


def bench_child(mode):
    if mode == "parent":
        as_parent()
    base.bench_child("default")


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"pitch_carry_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "path", "carry"]
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[pitch carry probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[pitch carry probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["carry_over_path_ms"] = round(res["carry_p50_ms"] - res["path_p50_ms"], 4)
    res["carry_vs_path"] = round(res["carry_p50_ms"] / res["path_p50_ms"] - 1.0, 5)
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "pitch_carry_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("pitch_carry_probe: a stream or a bench step without the path is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
