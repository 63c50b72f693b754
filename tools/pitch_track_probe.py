"""What does tracking every stream's pitch register cost per block?  (Not part of the bench; run on the GPU box.)

BASELINE configs[2]'s 32 streams (bench_stream.py's loop: 1920-sample blocks, 13 440-sample buffers, a 1000-vector index, use_graph=True),
220 blocks after 20 warm-up blocks, p50 / p95 of the block latency:
  untracked          BatchedStreamInfer as it was: this tree's library, and - with `--parent-lib PATH`, a build of the parent commit - that
                     library too, each in fresh processes that take turns (tools/ab_latency.sh's scheme), twice each
  tracked            BatchedStreamInfer(auto_pitch=[S] registers): tvc_convert_track_f32, the tracker's launch in the place of none
and the tracker's launch alone (tvc_pitch_track_f32 over f0 [S, 28], W = 1500, rings filled, hipEvent time over 200 launches) at S = 32
and S = 4096.
Gate: the untracked p50 of this tree within 3 % of the parent library's (the pool's box-to-box spread, README).  The tracked figure is
recorded, not gated: there is no earlier number to hold it against.
Writes profiles/pitch_track_probe.json and prints it as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, BLOCKS, WARM = 32, 240, 20
NEW_ENTRIES = ("tvc_pitch_track_f32", "tvc_convert_track_f32")


def child(mode):
    """one stream run in this process -> {"p50_ms", "p95_ms"} as a JSON line"""
    import numpy as np
    import torch
    from tinyvc_amd import _lib
    if mode == "parent":      # the parent commit's library has every entry but the two new ones, which the untracked path never calls
        for name in NEW_ENTRIES:
            _lib.SIGNATURES.pop(name, None)
    import bench
    from tinyvc_amd import synth
    from tinyvc_amd.module.infer import BatchedStreamInfer
    dev = torch.device("cuda", 0)
    gen = bench.build_generator(dev)
    S = STREAMS
    kw = dict(auto_pitch=torch.full((S,), 220.0, device=dev)) if mode == "tracked" else {}
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, block_size=1920, extra_size=3840, use_graph=True, **kw)
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
    assert torch.isfinite(out).all()
    l = np.sort(np.array(lat[WARM:])) * 1e3
    res = {"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)])}
    if mode == "tracked":
        res["voiced_frames_tracked"] = int(st.pitch_track.count.sum())
        res["shift_min"], res["shift_max"] = float(st.last_pitch_shift.min()), float(st.last_pitch_shift.max())
    print(json.dumps(res))


def kernel_ms(S, W=1500, T=28, launches=200):
    """the tracker's launch alone, rings full: milliseconds per launch by hipEvents around `launches` of them"""
    import torch
    from tinyvc_amd.engine import default_engine
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    dev = torch.device("cuda", 0)
    eng = default_engine(dev)
    tr = PitchTrack(S, 4, lag_frames=8, window_frames=W, device=dev)
    tr.ring.uniform_(80.0, 400.0)
    tr.count.fill_(10 * W)
    f0 = torch.empty(S, T, device=dev).uniform_(80.0, 400.0)
    target = torch.full((S,), 220.0, device=dev)
    for _ in range(10):
        eng.pitch_track(f0, tr, target, want_shifted=True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(launches):
        eng.pitch_track(f0, tr, target, want_shifted=True)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / launches


def main():
    if "--child" in sys.argv:
        return child(sys.argv[sys.argv.index("--child") + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["untracked", "tracked"]
    runs = {m: [] for m in modes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            env = dict(os.environ)
            if m == "parent":
                env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
            if out.returncode != 0:
                sys.exit(f"pitch_track_probe: the {m} run failed:\n{out.stdout}{out.stderr}")
            runs[m].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"[pitch track probe] {m}: {runs[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["tracked"] = {k: runs["tracked"][-1][k] for k in ("voiced_frames_tracked", "shift_min", "shift_max")}
    if parent_lib:
        res["untracked_vs_parent"] = round(res["untracked_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["untracked_within_3_percent_of_parent"] = bool(abs(res["untracked_vs_parent"]) <= 0.03)
    for S in (32, 4096):
        res[f"kernel_s{S}_w1500_ms"] = round(kernel_ms(S), 5)
    with open(os.path.join(ROOT, "profiles", "pitch_track_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["untracked_within_3_percent_of_parent"]:
        sys.exit("pitch_track_probe: the untracked stream is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
