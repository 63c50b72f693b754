"""What does finding the pitch shift on the device cost?  (Not part of the bench; run on the GPU box.)

BASELINE configs[1]'s batch (64 utterances x 4 s, one shared 10 000-vector index as a per-row table) and a B = 1 call of the same length:
  explicit   tvc_convert_multi_f32 with one host shift per row (the route the parent commit has: `--explicit-only` runs it alone, so a
             checkout of the parent gives its own figure on the same box)
  auto       tvc_convert_auto_f32: the same call, the shifts found by pitch_match_kernel between the encoder and the decoder
and the register of ONE row of 4 000 000 frames (an index build's packed f0; offline, no gate).
The routes alternate in one process, round robin: every figure is the median of 20 rounds after 3 warm-up rounds, with min and max.
Gate: auto <= explicit + max(3 % of explicit, the explicit route's own max - min) - 3 % is the pool's box-to-box spread (README), and the
new launch is one dependent kernel of at most a few hundred workgroups.
Writes profiles/auto_pitch_probe.json and prints it as one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from tinyvc_amd import synth  # noqa: E402
from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_reference  # noqa: E402

ROUNDS, WARM = 20, 3


def alternate(routes, rounds=ROUNDS, warm=WARM):
    """{name: fn} -> {name: (median, min, max) ms}; the routes take turns inside every round, so drift of the box hits all of them alike"""
    ts = {k: [] for k in routes}
    for r in range(warm + rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def main():
    explicit_only = "--explicit-only" in sys.argv
    dev = torch.device("cuda:0")
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    L, N = 4 * 24000, 10000
    blob, n = prepare_reference(synth.synth_index(N, seed=8).to(dev))
    res = {}
    for B in (64, 1):
        wf = synth.synth_wave(B, L, seed=100).to(dev)
        angle = synth.synth_angle(B, L // 480, 3).to(dev)
        shifts = [0.25 * (b % 9) - 1.0 for b in range(B)]
        routes = {"explicit": lambda wf=wf, angle=angle, shifts=shifts, B=B: eng.convert_multi(wf, [blob] * B, [n] * B, shifts, angle)}
        if not explicit_only:
            target = torch.full((B,), 220.0, device=dev)
            routes["auto"] = lambda wf=wf, angle=angle, shifts=shifts, B=B, target=target: eng.convert_auto(wf, [blob] * B, [n] * B, target, shifts, None, angle)
        t = alternate(routes)
        for k, (med, lo, hi) in t.items():
            res[f"b{B}_{k}_ms"], res[f"b{B}_{k}_min_ms"], res[f"b{B}_{k}_max_ms"] = med, lo, hi
        if not explicit_only:
            allowed = t["explicit"][0] + max(0.03 * t["explicit"][0], t["explicit"][2] - t["explicit"][1])
            res[f"b{B}_allowed_ms"] = allowed
            res[f"b{B}_within_gate"] = bool(t["auto"][0] <= allowed)
    if explicit_only:
        print(json.dumps({k: round(v, 4) for k, v in res.items()}))
        return
    S = 4_000_000
    f0 = torch.exp(torch.empty(S, device=dev).uniform_(3.0, 8.0))
    f0[torch.rand(S, device=dev) < 0.2] = 0.0
    med, lo, hi = alternate({"register": lambda: eng.pitch_match(f0, [0, S])})["register"]
    res["row_4m_frames_register_ms"], res["row_4m_frames_register_min_ms"], res["row_4m_frames_register_max_ms"] = med, lo, hi
    res = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}
    res["config"] = {"batches": [64, 1], "seconds": 4, "index_vectors": N, "rounds": ROUNDS, "warmup": WARM, "long_row_frames": S}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "auto_pitch_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (res["b64_within_gate"] and res["b1_within_gate"]):
        sys.exit("auto_pitch_probe: the automatic route is outside its gate")


if __name__ == "__main__":
    main()
