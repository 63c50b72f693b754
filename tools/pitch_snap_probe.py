"""What does pitch correction cost, and does a stream or a call without it cost what it did?  (Not part of the bench; run on the GPU box.)

Fresh processes that take turns (tools/pitch_carry_probe.py's scheme), twice each, the best figure of the two:
  streams   BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, a 1000-vector index, use_graph=True), 220 blocks
            after 20 warm-up blocks, p50 / p95 of the block latency: this tree's library without `tune` (`default`), with
            `--parent-lib PATH` - a build of the parent commit - that library too (`parent`), and this tree's with tune="C major" (`tune`:
            one more launch in the captured graph, in front of the decoder, and the state of 32 streams carried in place)
  bench     bench.py's headline (`--gpus 1 --steps 10 --warmup 3`, the timed steps alone) with either library
  kernels   by hipEvents: the 64 x 4 s batch with and without tune, and the stage launch alone (the entry on buffers made once) at 64 x 200,
            32 x 28, 4 096 x 28 and 1 x 15 000 frames of a wandering, partly unvoiced f0
The one condition: `default` p50 and the bench headline of this tree within 3 % of the parent library's (the pool's box-to-box spread,
README) - a stream or a call without tune launches what it launched before.  Everything about `tune` is recorded, not gated.
Writes profiles/pitch_snap_probe.json and prints it as one JSON line."""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pitch_path_probe as base  # noqa: E402  (its bench child, its event timer and its constants are this probe's too)

STREAMS, BLOCKS, WARM = base.STREAMS, base.BLOCKS, base.WARM
NEW_ENTRIES = ("tvc_pitch_snap_f32", "tvc_tuned_convert_f32", "tvc_tuned_convert_ragged_f32")
STREAM_KW = {"parent": {}, "default": {}, "tune": {"tune": "C major"}}


def as_parent():
    """the parent commit's library has every entry but the new ones, which a stream or a call without tune never reaches"""
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
    res = {}
    if mode == "tune":      # the state did travel: it is no longer the fresh one everywhere
        res["streams_on_a_note"] = int((st.tune_carry.note >= 0).sum())
    l = np.sort(np.array(lat[WARM:])) * 1e3
    print(json.dumps(dict(res, p50_ms=float(l[len(l) // 2]), p95_ms=float(l[int(len(l) * 0.95)]))))


def bench_child(mode):
    if mode == "parent":
        as_parent()
    base.bench_child("default")


def kernel_child(_mode):
    """the batch with and without tune, and the stage launch alone: milliseconds per call by hipEvents"""
    import numpy as np
    import torch
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchSnap
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    res = {}
    B, L = 64, 4 * 24000
    wf = synth.synth_wave(4, L, seed=300)[torch.arange(B) % 4].to(dev).contiguous()
    tgt = [synth.synth_index(1000, seed=2).to(dev)] * B
    angle = synth.synth_angle(1, L // 480, 5).to(dev).expand(B, -1, -1).contiguous()
    tune = PitchSnap()
    res["batch_64x4s_ms"] = base._events_ms(lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle), 20)
    res["batch_64x4s_tune_ms"] = base._events_ms(lambda: gen.convert(wf, tgt, 0.0, noise_angle=angle, tune=tune), 20)
    res["batch_64x4s_tune_over_plain"] = res["batch_64x4s_tune_ms"] / res["batch_64x4s_ms"] - 1.0
    settings = tune.settings()
    for rows, T in base.STAGE_SHAPES:      # the entry itself on buffers made once: Engine.pitch_snap would add two allocations
        r = np.random.default_rng(rows)
        f0 = 220.0 * 2.0 ** (np.cumsum(r.normal(0, 25, (rows, T)), axis=1) / 1200.0 + r.uniform(-1, 1, (rows, 1)))      # a melody that wanders through notes
        f0[r.random((rows, T)) < 0.1] = 0.0
        x = torch.from_numpy(f0.astype(np.float32)).to(dev)
        out, note = torch.empty_like(x), torch.empty(rows, T, dtype=torch.int32, device=dev)
        tune.bind(dev, rows)
        I64 = ctypes.c_int64 * rows
        start, count = I64(*(b * T for b in range(rows))), I64(*([T] * rows))

        def launch():
            eng._ok(eng.lib.tvc_pitch_snap_f32(eng.ctx, eng._stream(), x.data_ptr(), start, count, rows, ctypes.byref(settings), tune.notes.data_ptr(),
                                               tune.strength.data_ptr(), 0, None, None, out.data_ptr(), note.data_ptr()), "tvc_pitch_snap_f32")
        res[f"stage_{rows}x{T}_ms"] = base._events_ms(launch, 20, warm=2)
        res[f"stage_{rows}x{T}_notes_changed"] = int((note[:, 1:] != note[:, :-1]).sum())
    res["stage_1x15000_us_per_frame"] = res["stage_1x15000_ms"] * 1e3 / 15000
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"pitch_snap_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--stream-child", stream_child), ("--bench-child", bench_child), ("--kernel-child", kernel_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "tune"]
    bmodes = (["parent"] if parent_lib else []) + ["default"]
    runs, bruns = {m: [] for m in modes}, {m: [] for m in bmodes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--stream-child", m, parent_lib))
            print(f"[pitch snap probe] streams {m}: {runs[m][-1]}", flush=True)
        for m in bmodes:
            bruns[m].append(run_child("--bench-child", m, parent_lib))
            print(f"[pitch snap probe] bench {m}: {bruns[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["tune_streams_on_a_note"] = runs["tune"][-1]["streams_on_a_note"]
    res["tune_over_default_ms"] = round(res["tune_p50_ms"] - res["default_p50_ms"], 4)
    res["tune_vs_default"] = round(res["tune_p50_ms"] / res["default_p50_ms"] - 1.0, 5)
    for m in bmodes:
        res[f"bench_{m}_value"] = round(max(r["value"] for r in bruns[m]), 1)
        res[f"bench_{m}_runs"] = [round(r["value"], 1) for r in bruns[m]]
    res.update(run_child("--kernel-child", "default", parent_lib))
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["bench_vs_parent"] = round(res["bench_default_value"] / res["bench_parent_value"] - 1.0, 5)
        res["within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03 and abs(res["bench_vs_parent"]) <= 0.03)
    with open(os.path.join(ROOT, "profiles", "pitch_snap_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["within_3_percent_of_parent"]:
        sys.exit("pitch_snap_probe: a stream or a bench step without tune is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
