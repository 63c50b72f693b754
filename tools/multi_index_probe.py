"""What does one index per utterance cost?  (Not part of the bench; run on the GPU box.)

BASELINE configs[1] (64 utterances x 4 s, 10 000-vector indices) three ways:
  shared   one index for every row: Generator.convert -> tvc_convert_f32 (the bench's step)
  multi    64 distinct indices: tvc_convert_multi_f32 (one call, segment plan)
  staged   64 distinct indices through the staged path the multi call replaces: STFT, energy, encoder, one knn_match per row,
           shift, decoder
and the 32-stream block latency (configs[2], 1 000-vector indices, HIP-graph replay) with 32 distinct indices next to one shared index.
Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from tinyvc_amd import synth  # noqa: E402
from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_reference, prepare_references  # noqa: E402


def timed(fn, steps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def stream_p50(gen, dev, target, streams=32, blocks=60, warmup=12):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=streams, target=target, device=dev, block_size=1920, extra_size=3840, use_graph=True)
    st.init_buffer()
    waves = torch.stack([synth.synth_wave(1, blocks * 1920, seed=200 + s)[0] for s in range(4)])
    waves = waves[torch.arange(streams) % 4].to(dev).view(streams, blocks, 1920)
    lat = []
    for i in range(blocks):
        blk = waves[:, i].contiguous()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        st.audio_callback(blk)
        torch.cuda.synchronize(dev)
        lat.append((time.perf_counter() - t0) * 1e3)
    lat = sorted(lat[warmup:])
    return lat[len(lat) // 2]


def main():
    dev = torch.device("cuda:0")
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    B, L, N = 64, 4 * 24000, 10000
    wf = synth.synth_wave(B, L, seed=100).to(dev)
    shared = synth.synth_index(N, seed=8).to(dev)
    distinct = [synth.synth_index(N, seed=1000 + b).to(dev) for b in range(B)]
    blob, n = prepare_reference(shared)
    blobs, ns = prepare_references(distinct)
    angle = synth.synth_angle(B, L // 480, 3).to(dev)

    def staged():
        spec = eng.stft_mag(wf)
        energy = eng.energy(wf)
        z, f0, _ = eng.encoder(spec)
        z = torch.cat([eng.knn_match(z[b:b + 1], blobs[b], ns[b]) for b in range(B)], 0)
        f0 = eng.shift_frequency(f0, 0.0)
        return eng.decoder(z, f0, energy, angle)

    res = {
        "shared_ms": timed(lambda: eng.convert(wf, blob, n, 0.0, angle)),
        "multi_ms": timed(lambda: eng.convert_multi(wf, blobs, ns, 0.0, angle)),
        "staged_ms": timed(staged, steps=5, warm=2),
    }
    res["multi_over_shared"] = res["multi_ms"] / res["shared_ms"]
    s_shared = synth.synth_index(1000, seed=2).to(dev)
    s_distinct = [synth.synth_index(1000, seed=2000 + s).to(dev) for s in range(32)]
    res["stream32_shared_p50_ms"] = stream_p50(gen, dev, s_shared)
    res["stream32_distinct_p50_ms"] = stream_p50(gen, dev, s_distinct)
    res["stream_over_shared"] = res["stream32_distinct_p50_ms"] / res["stream32_shared_p50_ms"]
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == "__main__":
    main()
