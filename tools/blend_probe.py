"""What does converting toward a weighted blend of indices cost?  (Not part of the bench; run on the GPU box.)

BASELINE configs[1]'s batch (64 utterances x 4 s, 10 000-vector indices):
  single    one index for every row: tvc_convert_f32 (the bench's step)
  blend M   tvc_convert_blend_f32 with M = 1, 2 and 4 shared 10 000-vector indices
  staged    the M = 2 blend through the staged route the call replaces: STFT, energy, encoder, one knn_match per term, a torch
            blend, shift, decoder - only entries the parent commit has, so `--staged-only` runs against a parent checkout too
and the 32-stream block latency (configs[2]: 1 000-vector indices, HIP-graph replay) with one shared index and with an M = 2 blend.
The routes alternate in one process, round robin: every figure is the median of 20 rounds after 3 warm-up rounds.
Writes profiles/blend_probe.json (`--staged-only`: prints the staged figure alone and writes nothing) and prints it as one JSON line."""
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
    """{name: fn} -> {name: median ms}; the routes take turns inside every round, so drift of the box hits all of them alike"""
    ts = {k: [] for k in routes}
    for r in range(warm + rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def stream_p50(gen, dev, targets, streams=32, rounds=ROUNDS, warm=12):
    """{name: target} -> {name: p50 block ms}: one BatchedStreamInfer per target under graph replay, fed the same blocks in turns"""
    from tinyvc_amd.module.infer import BatchedStreamInfer
    blocks = warm + rounds
    waves = torch.stack([synth.synth_wave(1, blocks * 1920, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(streams) % 4].to(dev).view(streams, blocks, 1920)
    sts, lat = {}, {k: [] for k in targets}
    for k, tgt in targets.items():
        sts[k] = BatchedStreamInfer(gen, n_streams=streams, target=tgt, device=dev, block_size=1920, extra_size=3840, use_graph=True)
        sts[k].init_buffer()
    for i in range(blocks):
        blk = waves[:, i].contiguous()
        for k, st in sts.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st.audio_callback(blk)
            torch.cuda.synchronize(dev)
            if i >= warm:
                lat[k].append((time.perf_counter() - t0) * 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in lat.items()}


def main():
    staged_only = "--staged-only" in sys.argv
    dev = torch.device("cuda:0")
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    B, L, N = 64, 4 * 24000, 10000
    wf = synth.synth_wave(B, L, seed=100).to(dev)
    idx = [synth.synth_index(N, seed=8 + m).to(dev) for m in range(4)]
    prepared = [prepare_reference(t) for t in idx]
    angle = synth.synth_angle(B, L // 480, 3).to(dev)
    w2 = torch.tensor([0.7, 0.3], device=dev)

    def staged():
        spec = eng.stft_mag(wf)
        energy = eng.energy(wf)
        z, f0, _ = eng.encoder(spec)
        zm = w2[0] * eng.knn_match(z, *prepared[0]) + w2[1] * eng.knn_match(z, *prepared[1])
        f0 = eng.shift_frequency(f0, 0.0)
        return eng.decoder(zm, f0, energy, angle)

    if staged_only:
        print(json.dumps({"staged_m2_ms": round(alternate({"staged": staged})["staged"], 4)}))
        return
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    routes = {"single_ms": lambda: eng.convert(wf, *prepared[0], 0.0, angle), "staged_m2_ms": staged}
    for M, w in ((1, [1.0]), (2, [0.7, 0.3]), (4, [0.4, 0.3, 0.2, 0.1])):
        blobs, ns, wd = Blend(idx[:M], w).resolve(B, dev)
        routes[f"blend_m{M}_ms"] = lambda blobs=blobs, ns=ns, wd=wd: eng.convert_blend(wf, blobs, ns, wd, 0.0, angle)
    res = alternate(routes)
    res["blend_m1_over_single"] = res["blend_m1_ms"] / res["single_ms"]
    res["blend_m2_over_single"] = res["blend_m2_ms"] / res["single_ms"]
    res["blend_m4_over_single"] = res["blend_m4_ms"] / res["single_ms"]
    res["staged_m2_over_blend_m2"] = res["staged_m2_ms"] / res["blend_m2_ms"]
    s_idx = [synth.synth_index(1000, seed=2 + m).to(dev) for m in range(2)]
    p50 = stream_p50(gen, dev, {"stream32_shared_p50_ms": s_idx[0], "stream32_blend_m2_p50_ms": Blend(s_idx, [0.7, 0.3])})
    res.update(p50)
    res["stream_blend_m2_over_shared"] = p50["stream32_blend_m2_p50_ms"] / p50["stream32_shared_p50_ms"]
    res = {k: round(v, 4) for k, v in res.items()}
    res["config"] = {"batch": B, "seconds": 4, "index_vectors": N, "rounds": ROUNDS, "warmup": WARM, "streams": 32, "stream_index_vectors": 1000}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "blend_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
