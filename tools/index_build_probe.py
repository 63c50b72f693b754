"""What does building a speaker index on the device cost?  (Not part of the bench; run on one MI355X, one process holding the GPU.)

  gather    tvc_knn_prepare_index_cols_f32 (one launch: gather + prepare) against the two-step route it replaces -
            torch.index_select(feats, 1, cols) followed by tvc_knn_prepare_index_f32 - at N = 10 000 and 100 000, S = 4 N, random cols.
            The two routes alternate inside one process; every figure is the median of 20 calls after 3 warm-ups, each call timed from
            enqueue to stream synchronise.  `spread` is the two-step route's own max - min over its 20 calls.
  encode    256 clips of 100 frames through build_index (one ragged encode, column plan, one gather) against the clip-by-clip loop:
            Generator.encode per clip, .cpu(), host assemble, upload, knn_prepare.  No file I/O on either side.
Prints one JSON line (kept under profiles/)."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from tinyvc_amd import synth  # noqa: E402
from tinyvc_amd.module.tinyvc import build_index  # noqa: E402

STEPS, WARM = 20, 3


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


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


def gather_case(eng, N):
    dev = eng.device
    S = 4 * N
    g = torch.Generator().manual_seed(N)
    feats = torch.randn(768, S, generator=g).to(dev)
    cols = torch.randint(0, S, (N,), generator=g).to(dev)
    lib = eng.lib
    blob_a = torch.empty(lib.tvc_knn_prepared_elems(N), device=dev)
    blob_b = torch.empty_like(blob_a)
    out = torch.empty(768, N, device=dev)

    def two_step():
        sel = torch.index_select(feats, 1, cols)
        eng._ok(lib.tvc_knn_prepare_index_f32(eng.ctx, eng._stream(), _ptr(sel), _ptr(blob_a), N), "tvc_knn_prepare_index_f32")

    def gather():
        eng._ok(lib.tvc_knn_prepare_index_cols_f32(eng.ctx, eng._stream(), _ptr(feats), S, _ptr(cols), N, _ptr(blob_b), _ptr(out)),
                "tvc_knn_prepare_index_cols_f32")

    ts = alternate({"two_step": two_step, "gather": gather})
    same = bool(torch.equal(blob_a.view(torch.int32), blob_b.view(torch.int32)))
    for b in (blob_a, blob_b):
        lib.tvc_knn_forget(eng.ctx, _ptr(b))
    r = {"N": N, "S": S, "two_step": stats(ts["two_step"]), "gather": stats(ts["gather"]), "same_bytes": same}
    r["spread_ms"] = round(ts["two_step"][-1] - ts["two_step"][0], 4)
    r["gather_over_two_step"] = round(r["gather"]["median_ms"] / r["two_step"]["median_ms"], 4)
    r["within_spread"] = r["gather"]["median_ms"] <= r["two_step"]["median_ms"] + r["spread_ms"]
    return r


def encode_case(gen, dev, clips=256, frames=100, stride=4):
    eng = gen.engine(dev)
    L = frames * 480
    wf = torch.stack([synth.synth_wave(1, L, seed=300 + b % 8)[0] for b in range(clips)]).to(dev)
    lens = [L] * clips
    supply = clips * -(-frames // stride)
    perm = torch.randperm(supply, generator=torch.Generator().manual_seed(7))

    def loop():
        feats = [gen.encode(wf[b:b + 1])[0].cpu()[:, :, ::stride] for b in range(clips)]
        tgt = torch.cat(feats, dim=2).index_select(2, perm).contiguous()
        return tgt, eng.knn_prepare(tgt.to(dev))

    def batched():
        return build_index(gen, wf, lens, stride=stride, perm=perm)

    ts = alternate({"loop": loop, "batched": batched})
    same = bool(torch.equal(loop()[0], batched().cpu()))
    r = {"clips": clips, "frames": frames, "vectors": supply, "loop": stats(ts["loop"]), "batched": stats(ts["batched"]), "same_index": same}
    r["loop_over_batched"] = round(r["loop"]["median_ms"] / r["batched"]["median_ms"], 2)
    return r


def main():
    dev = torch.device("cuda:0")
    gen = bench.build_generator(dev)
    eng = gen.engine(dev)
    res = {"steps": STEPS, "warmup": WARM, "gather": [gather_case(eng, N) for N in (10000, 100000)], "encode": encode_case(gen, dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
