"""What does compacting a speaker index on the device cost, and what does it buy?  (Not part of the bench; run on one MI355X, one process
holding the GPU.)  Writes profiles/index_compact_probe.json and prints the same JSON line.

  iteration  one k-means iteration split into its stages - assign (tvc_index_assign_f32), update (tvc_index_update_f32), prepare
             (tvc_knn_prepare_index_f32 of the centroids) - at N = 100 000 -> K = 10 000 with fp32 points and N = 1 000 000 -> K = 10 000
             and 100 000 with fp16 points.  Beside the update: the same update done by torch on the same GPU (zeros [K, 768],
             index_add_ of the fp32 rows, a divide by the clamped counts, a transpose into [768, K]); torch reads an fp32 copy of the
             rows whatever the blob stores.  The two updates alternate inside one process; every figure is the median of 20 calls after
             3 warm-ups, each call timed from enqueue to stream synchronise.
  bandwidth  the update's point bytes (N x 768 x 4 or 2) over its median time, beside the 4.8 TB/s of a copy kernel (DESIGN.md
             section 8): whether the fp64 adds or the row gather limit it.
  payoff     configs[3]'s batch (64 x 4 s) converted against a 100 000-vector index and against its 10 000-centroid compaction (8
             iterations), alternating in the same process.
  agreement  the mean cosine between the matched features of the two indices, on held-out queries drawn from the same mixture.
The points are a planted mixture (64 centres, sigma 0.5): k-means of unstructured noise says nothing about a speaker's frames."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from tinyvc_amd import synth  # noqa: E402
from tinyvc_amd.module.tinyvc import compact_index, match_features  # noqa: E402

STEPS, WARM = 20, 3
COPY_TBS = 4.8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternate(fns, steps=STEPS, warm=WARM):
    """{name: sorted milliseconds}: the routes take turns, so drift of the box lands on all of them."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.current_stream().synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: sorted(v) for k, v in ts.items()}


def stats(v):
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def mixture(n, seed, dev, centres=64, sigma=0.5, dtype=torch.float32, piece=100000):
    """[768, n] on the device: n draws around `centres` planted centres (seed 1 fixes the centres, `seed` the draws)."""
    cen = torch.randn(centres, 768, generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(768, n, dtype=dtype, device=dev)
    for o in range(0, n, piece):
        m = min(piece, n - o)
        lab = torch.randint(0, centres, (m,), generator=g, device=dev)
        out[:, o:o + m] = (cen[lab] + sigma * torch.randn(m, 768, generator=g, device=dev)).t().to(dtype)
    return out


def iteration_case(eng, N, K, half):
    dev = eng.device
    pts = mixture(N, 10 + (N + K) % 97, dev, dtype=torch.float16 if half else torch.float32)
    blob, _ = eng.knn_prepare(pts)
    rows32 = pts.t().float().contiguous()                          # torch's operand: fp32 rows
    del pts
    init = torch.randperm(N, generator=torch.Generator().manual_seed(N + K))[:K].to(dev)
    cent = rows32[init].t().contiguous()
    cblob, _ = eng.knn_prepare(cent)
    assign, _s, _m = eng.index_assign(blob, N, cblob, K)
    lib = eng.lib
    ours = cent.clone()
    theirs = torch.empty_like(cent)

    def f_assign():
        eng.index_assign(blob, N, cblob, K, assign=assign)

    def f_update():
        eng.index_update(blob, N, assign, ours)

    def f_update_torch():
        sums = torch.zeros(K, 768, device=dev)
        sums.index_add_(0, assign, rows32)
        cnt = torch.bincount(assign, minlength=K).clamp_(min=1)
        theirs.copy_((sums / cnt[:, None]).t())

    def f_prepare():
        eng._ok(lib.tvc_knn_prepare_index_f32(eng.ctx, eng._stream(), ctypes.c_void_p(ours.data_ptr()), ctypes.c_void_p(cblob.data_ptr()), K), "tvc_knn_prepare_index_f32")

    ts = alternate({"assign": f_assign, "update": f_update, "update_torch": f_update_torch, "prepare": f_prepare}, steps=STEPS, warm=WARM)
    counts = torch.bincount(assign, minlength=K)
    nz = counts > 0
    diff = float((ours[:, nz] - theirs[:, nz]).abs().max())
    bytes_pts = N * 768 * (2 if half else 4)
    r = {"N": N, "K": K, "points": "fp16" if half else "fp32", "largest_cluster": int(counts.max()), "empty_clusters": int((~nz).sum()),
         "assign": stats(ts["assign"]), "update": stats(ts["update"]), "update_torch": stats(ts["update_torch"]), "prepare": stats(ts["prepare"]),
         "max_abs_diff_vs_torch": diff}
    r["iteration_ms"] = round(r["assign"]["median_ms"] + r["update"]["median_ms"] + r["prepare"]["median_ms"], 4)
    r["iteration_torch_update_ms"] = round(r["assign"]["median_ms"] + r["update_torch"]["median_ms"] + r["prepare"]["median_ms"], 4)
    r["update_TBps"] = round(bytes_pts / (r["update"]["median_ms"] * 1e-3) / 1e12, 4)
    r["update_over_copy_rate"] = round(r["update_TBps"] / COPY_TBS, 4)
    return r


def payoff_case(gen, dev, N=100000, K=10000, iters=8):
    big = mixture(N, 5, dev)[None].contiguous()
    t0 = time.perf_counter()
    small, info = compact_index(big, K, iters=iters, generator=torch.Generator().manual_seed(3), return_info=True)
    torch.cuda.synchronize()
    compact_ms = (time.perf_counter() - t0) * 1e3
    wf = synth.synth_wave(64, 96000, seed=1000).to(dev)
    angle = synth.synth_angle(64, 200, 5).to(dev)
    ts = alternate({"index_100k": lambda: gen.convert(wf, big, 0.0, noise_angle=angle), "compacted_10k": lambda: gen.convert(wf, small, 0.0, noise_angle=angle)})
    q = mixture(4096, 77, dev)[None].contiguous()                   # held out: draws the index never saw
    a, b = match_features(q, big), match_features(q, small)
    cos = torch.nn.functional.cosine_similarity(a[0], b[0], dim=0)
    sub = big[:, :, torch.randperm(N, generator=torch.Generator().manual_seed(3))[:K].to(dev)].contiguous()      # the recipe's way to 10 000: a random subsample
    c = match_features(q, sub)
    cos_sub = torch.nn.functional.cosine_similarity(a[0], c[0], dim=0)
    r = {"batch": "64 x 4 s", "N": N, "K": K, "iters": iters, "compact_ms_first_call": round(compact_ms, 2), "moved": info["moved"].tolist(),
         "convert_index_100k": stats(ts["index_100k"]), "convert_compacted_10k": stats(ts["compacted_10k"]),
         "matched_cosine_centroids_vs_full_mean": round(float(cos.mean()), 5), "matched_cosine_centroids_vs_full_min": round(float(cos.min()), 5),
         "matched_cosine_subsample_vs_full_mean": round(float(cos_sub.mean()), 5), "queries": 4096}
    r["speedup"] = round(r["convert_index_100k"]["median_ms"] / r["convert_compacted_10k"]["median_ms"], 3)
    return r


def main():
    dev = torch.device("cuda:0")
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    cases = [(100000, 10000, False), (1000000, 10000, True), (1000000, 100000, True)]
    if "--small" in sys.argv:                                       # a quick pass over the code path
        cases = cases[:1]
    res = {"steps": STEPS, "warmup": WARM, "copy_kernel_TBps": COPY_TBS, "iteration": []}
    for N, K, half in cases:
        res["iteration"].append(iteration_case(eng, N, K, half))
        torch.cuda.empty_cache()
    res["payoff"] = payoff_case(gen, dev)
    line = json.dumps(res)
    print(line)
    if "--small" not in sys.argv:
        with open(os.path.join(ROOT, "profiles", "index_compact_probe.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
