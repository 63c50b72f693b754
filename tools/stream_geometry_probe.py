"""What does a run-time SOLA geometry cost, and what does a short one leave of the block budget?  (Not part of the bench; run on the GPU box.)

BASELINE configs[2]'s 32 streams (bench_stream.py's loop: a 1000-vector index, use_graph=True), 220 blocks after 20 warm-up blocks, p50 / p95
of the block latency, in fresh processes that take turns (tools/stream_door_probe.py's scheme), twice each, best p50:
  default            the reference's geometry (1920 / 1920 / 3840, 1920-sample blocks, 13 440-sample windows): this tree's library, and - with
                     `--parent-lib PATH`, a build of the parent commit - that library too
  short              README.md's example: --crossfade 240 --sola-search 240 --lookahead 480 with 480-sample blocks and -e 3840 (4320-sample
                     windows): the per-block time against the 20 ms such a block lasts
and the tail alone - both SOLA launches (the split lag search and the arg-max / cross-fade / buffer update), hipEvent time over 200 calls -
at S = 32 and S = 1024 for the default geometry with either library, and for the short geometry with this tree's.
Gate: the default p50 of this tree within 3 % of the parent library's (the pool's box-to-box spread, README): the default geometry runs the
compile-time instantiation of the same kernels.  Everything else is recorded, not gated.
Writes profiles/stream_geometry_probe.json and prints it as one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, BLOCKS, WARM = 32, 240, 20
NEW_ENTRIES = ("tvc_sola_geometry", "tvc_sola_geometry_message", "tvc_sola_geom_f32")
SHORT = dict(crossfade_size=240, sola_search_size=240, last_delay_size=480, block_size=480)


def as_parent():
    """the parent commit's library has every entry but the new ones: the geometry check in plain Python, the tail through tvc_sola_f32"""
    from tinyvc_amd import _lib, engine
    from tinyvc_amd.module.infer import stream as stream_mod
    for name in NEW_ENTRIES:
        _lib.SIGNATURES.pop(name, None)
    stream_mod.sola_geometry = lambda b, c, s, d: (b + c + s + d, c + d, c + s + d)
    plain = engine.Engine.sola
    engine.Engine.sola = lambda self, y, buf, fade, block, pv=False, want_shift=False, **geometry: plain(self, y, buf, fade, block, pv, want_shift)


def child(mode):
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
    kw = SHORT if mode == "short" else dict(block_size=1920)
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(1000, seed=2).to(dev), device=dev, extra_size=3840, use_graph=True, **kw)
    st.init_buffer()
    chunk = st.block_size
    waves = torch.stack([synth.synth_wave(1, BLOCKS * chunk, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(S) % 4].to(dev).view(S, BLOCKS, chunk)
    lat = []
    for i in range(BLOCKS):
        blk = waves[:, i].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = st.audio_callback(blk)
        torch.cuda.synchronize(dev)
        lat.append(time.perf_counter() - t0)
    assert out.shape == (S, chunk) and bool(out.abs().max() > 0)
    l = np.sort(np.array(lat[WARM:])) * 1e3
    print(json.dumps({"p50_ms": float(l[len(l) // 2]), "p95_ms": float(l[int(len(l) * 0.95)]), "window": st.input_size}))


def tail_ms(eng, S, geometry, block, launches=200):
    """both SOLA launches: milliseconds per call by hipEvents around `launches` of them"""
    import torch
    dev = eng.device
    cross, search, delay = geometry
    y = 0.1 * torch.randn(S, block + cross + search + 2 * delay, device=dev)
    buf = 0.1 * torch.randn(S, cross, device=dev)
    fade = torch.sin(torch.pi * torch.arange(cross, device=dev) / cross / 2) ** 2
    kw = {} if geometry == (1920, 1920, 3840) else dict(crossfade=cross, search=search, delay=delay)
    for _ in range(10):
        eng.sola(y, buf, fade, block, **kw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(launches):
        eng.sola(y, buf, fade, block, **kw)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / launches


def tail_child(mode):
    import torch
    if mode == "parent":
        as_parent()
    from tinyvc_amd.engine import default_engine
    eng = default_engine(torch.device("cuda", 0))
    res = {}
    for S in (32, 1024):
        res[f"tail_default_s{S}_ms"] = round(tail_ms(eng, S, (1920, 1920, 3840), 1920), 5)
        if mode != "parent":
            res[f"tail_short_s{S}_ms"] = round(tail_ms(eng, S, (240, 240, 480), 480), 5)
    print(json.dumps(res))


def run_child(flag, mode, parent_lib):
    env = dict(os.environ)
    if mode == "parent":
        env["TVC_LIB_PATH"] = os.path.abspath(parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), flag, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if out.returncode != 0:
        sys.exit(f"stream_geometry_probe: the {mode} run ({flag}) failed:\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    for flag, fn in (("--child", child), ("--tail-child", tail_child)):
        if flag in sys.argv:
            return fn(sys.argv[sys.argv.index(flag) + 1])
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    modes = (["parent"] if parent_lib else []) + ["default", "short"]
    runs = {m: [] for m in modes}
    for _rep in range(2):
        for m in modes:      # fresh processes that take turns: drift of the box hits every build alike
            runs[m].append(run_child("--child", m, parent_lib))
            print(f"[stream geometry probe] {m}: {runs[m][-1]}", flush=True)
    res = {"streams": STREAMS, "blocks": BLOCKS - WARM, "hip_graph": True, "short_geometry": SHORT, "short_window": runs["short"][0]["window"]}
    for m in modes:
        res[f"{m}_p50_ms"] = round(min(r["p50_ms"] for r in runs[m]), 4)
        res[f"{m}_p95_ms"] = round(min(r["p95_ms"] for r in runs[m]), 4)
        res[f"{m}_p50_runs_ms"] = [round(r["p50_ms"], 4) for r in runs[m]]
    res["short_block_budget_ms"] = SHORT["block_size"] / 24.0
    res["short_p50_share_of_budget"] = round(res["short_p50_ms"] / res["short_block_budget_ms"], 4)
    if parent_lib:
        res["default_vs_parent"] = round(res["default_p50_ms"] / res["parent_p50_ms"] - 1.0, 5)
        res["default_within_3_percent_of_parent"] = bool(abs(res["default_vs_parent"]) <= 0.03)
        res["parent_tail"] = run_child("--tail-child", "parent", parent_lib)
    res["tail"] = run_child("--tail-child", "default", parent_lib)
    with open(os.path.join(ROOT, "profiles", "stream_geometry_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if parent_lib and not res["default_within_3_percent_of_parent"]:
        sys.exit("stream_geometry_probe: the default geometry is outside 3 % of the parent library's")


if __name__ == "__main__":
    main()
