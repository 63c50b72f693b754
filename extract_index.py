#!/usr/bin/env python3
"""Build a kNN speaker index (`index.pt`, FloatTensor [1, 768, size]) from a folder of target-speaker
audio with the GPU encoder: the reference's `extract_index.py` (same output format, reference
extract_index.py:43-58): encoder features of each clip, every `--stride`-th frame, concatenated,
randomly permuted along time, truncated to `-size`.

  python extract_index.py --dataset-cache DIR -encp models/encoder.pt -size 2048 -o models/index.pt

DIR holds `*.wav` clips (the reference's preprocess.py cache of `{i}.wav` files works as is).

Under a launcher (`python -m torch.distributed.run --nproc-per-node N extract_index.py ...`, WORLD_SIZE > 1) the clips the index needs
are encoded by N GPUs: the shuffled file order and the prefix of it that fills `-size` vectors are computed by every rank from the WAV
headers alone (a clip of n samples at 24 kHz contributes ceil(ceil(n / 480) / stride) vectors), the prefix is split over the ranks by
length (tinyvc_amd/parallel.py lpt_split), each rank encodes its clips on cuda:LOCAL_RANK, and ONE gather (RCCL) brings the features to
rank 0, which assembles them in the shuffled order, permutes, truncates and writes the file - the same bytes as the single-GPU run with
the same `--seed`.

`--batch-frames F` (single-process runs) builds the index in one pass on the device: the clips of the shuffled order go through the
encoder in ragged calls of at most F frames (Engine.encode_ragged: every clip over its own length, bit-identical to its own call), the
features stay on the device, and ONE gather selects the strided, permuted, truncated columns (feature_retrieval.index_columns) - the same
bytes as the default clip-by-clip run with the same `--seed`, without a host round trip per clip.

`--compact K` compacts the index built by any of these routes to K vectors by k-means on the device (feature_retrieval.compact_index:
cosine assignment, raw-mean update, `--compact-iters` rounds, started from K vectors drawn from the same generator) instead of
truncating further: `-size` then sets how much of the speaker's material the centroids summarise.  `--compact-snap` replaces every
centroid by its nearest real frame.  Without `--compact` the file is what it always was.

Beside the index every route writes `<output>.f0.pt`: {"median_hz", "voiced"}, the speaker's pitch register - the lower median of the voiced
f0 of every frame of the clips the index was drawn from (feature_retrieval.pitch_register, on the device) - which `infer.py --auto-pitch`
and `infer_streaming.py --auto-pitch-from` aim at.  `index.pt` itself keeps the reference's format byte for byte.
"""
import argparse
import glob
import os
import sys

import torch

from tinyvc_amd import audio_io, parallel
from tinyvc_amd.module import utils
from tinyvc_amd.module.tinyvc import Encoder
from tinyvc_amd.module.tinyvc.feature_retrieval import compact_index, index_columns, index_from_columns, pitch_register, save_register, sidecar_path

SAMPLE_RATE = 24000


def encode_clip(enc, device, path, stride, f0_out=None):
    """[1, 768, ceil(T / stride)] on the CPU: the encoder's features of one clip, every `stride`-th frame (extract_index.py:47-52).
    f0_out (a list): the clip's f0 [T], all frames, is appended to it and stays on the device."""
    wf, sr = audio_io.load(path)
    wf = enc.engine(device).resample(wf.to(device), sr, SAMPLE_RATE).mean(dim=0, keepdim=True)
    spec = utils.spectrogram(utils.autopad_waveform(wf), enc.n_fft, enc.hop_size)
    z, f0 = enc.infer(spec)
    if f0_out is not None:
        f0_out.append(f0.reshape(-1))
    return z.cpu()[:, :, ::stride]


def clip_columns(path, stride, engine=None):
    """Index vectors a clip will contribute, from its header alone: frames at 24 kHz (the resampler's output length), padded to whole
    480-sample frames, every `stride`-th one."""
    frames, sr, _ch = audio_io.info(path)
    if sr != SAMPLE_RATE:
        frames = engine.lib.tvc_resample_out_len(frames, sr, SAMPLE_RATE) if engine is not None else -(-frames * SAMPLE_RATE // sr)
    t = -(-frames // 480)
    return -(-t // stride)


def needed_prefix(cols, order, size):
    """The reference's loop (extract_index.py:47-55) takes clips in shuffled order until MORE than `size` vectors are collected: the number
    of clips of `order` it ends up using."""
    total = 0
    for k, i in enumerate(order):
        total += cols[i]
        if total > size:
            return k + 1
    return len(order)


def sharded_features(cols, order, size, world, rank, encode, device, group=None):
    """The clips of the shuffled order's needed prefix, encoded by `world` ranks and gathered on rank 0 (the job's one exchange): returns
    the features in prefix order there, None elsewhere.  cols[i] = vectors clip i will contribute (header-derived: every rank computes the
    same prefix and the same split on its own), encode(i) -> [1, 768, cols[i]] on the CPU."""
    import torch.distributed as dist
    prefix = order[:needed_prefix(cols, order, size)]
    split = parallel.lpt_split([cols[i] for i in prefix], world)             # positions in `prefix`, per rank
    local = [encode(prefix[k]) for k in split[rank]]
    for k, z in zip(split[rank], local):
        if tuple(z.shape) != (1, 768, cols[prefix[k]]):
            raise RuntimeError(f"clip {prefix[k]}: features {tuple(z.shape)}, its header promised {cols[prefix[k]]} vectors")
    share = [sum(cols[prefix[k]] for k in split[r]) for r in range(world)]
    buf = torch.zeros(768, max(max(share), 1), device=device)
    if local:
        buf[:, :share[rank]] = torch.cat(local, dim=2)[0].to(device)
    parts = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
    dist.gather(buf, parts, dst=0, group=group)
    if rank != 0:
        return None
    feats = [None] * len(prefix)
    for r in range(world):
        off = 0
        for k in split[r]:
            n = cols[prefix[k]]
            feats[k] = parts[r][None, :, off:off + n].cpu()
            off += n
    return feats


def register_of(f0_parts):
    """the pitch register of every frame in f0_parts (device tensors) as one row"""
    f0 = f0_parts[0] if len(f0_parts) == 1 else torch.cat(f0_parts)
    return pitch_register(f0, [f0.numel()])


def gathered_register(f0_parts, world, rank, device, group=None):
    """The sharded run's register: every rank's f0 gathered on rank 0 (a median does not care for the order) and measured there as one row;
    None on the other ranks, and on rank 0 when the gathered f0 does not fit (the sidecar is then left out)."""
    import torch.distributed as dist
    local = torch.cat(f0_parts) if f0_parts else torch.zeros(0, device=device)
    n = torch.tensor([local.numel()], dtype=torch.int64, device=device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(x.item()) for x in sizes]
    try:
        buf = torch.zeros(max(max(sizes), 1), device=device)
        buf[:local.numel()] = local
        parts = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
    except torch.cuda.OutOfMemoryError:
        buf = parts = None
    ok = torch.tensor([0 if buf is None else 1], dtype=torch.int64, device=device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    if int(ok.item()) == 0:
        return None
    dist.gather(buf, parts, dst=0, group=group)
    if rank != 0:
        return None
    return register_of([parts[r][:sizes[r]] for r in range(world)])


def batched_index(enc, device, files, order, stride, size, gen, half, batch_frames, f0_out=None):
    """The default loop's index ([1, 768, size] on the CPU, the same bytes) with the clips encoded in ragged calls of at most `batch_frames`
    frames (a longer clip is a call of its own) and the selection done by one gather on the device."""
    eng = enc.engine(device)
    feats, frames, total = [], [], 0
    group, group_frames = [], 0

    def flush():
        if not group:
            return
        wf = torch.zeros(len(group), max(c.numel() for c in group), device=device)
        for r, c in enumerate(group):
            wf[r, :c.numel()] = c
        ssl, f0, _pre = eng.encode_ragged(wf, [c.numel() for c in group])
        feats.append(ssl)
        if f0_out is not None:
            f0_out.append(f0)
        group.clear()

    for i in order:
        wf, sr = audio_io.load(files[i])
        wf = utils.autopad_waveform(eng.resample(wf.to(device), sr, SAMPLE_RATE).mean(dim=0, keepdim=True))
        t = wf.shape[1] // 480
        if group and group_frames + t > batch_frames:
            flush()
            group_frames = 0
        group.append(wf[0])
        group_frames += t
        frames.append(t)
        total += -(-t // stride)
        if total > size:
            break
    flush()
    packed = feats[0] if len(feats) == 1 else torch.cat(feats, dim=1)
    cols = index_columns(frames, stride, size, torch.randperm(total, generator=gen))
    return index_from_columns(eng, packed, cols, half).cpu()


def assemble(feats_in_order, size, gen, half):
    feats = torch.cat(feats_in_order, dim=2)
    perm = torch.randperm(feats.shape[2], generator=gen)
    tgt = feats.index_select(2, perm)[:, :, :size].contiguous()
    return tgt.half() if half else tgt


def compacted(tgt, device, k, iters, snap, gen, half):
    """The index `tgt` ([1, 768, n] on the CPU, fp32) compacted to k centroids on the device; the start vectors come from `gen`."""
    if k > tgt.shape[2]:
        sys.exit(f"--compact {k}: the index holds only {tgt.shape[2]} vectors")
    out = compact_index(tgt.to(device), k, iters=iters, generator=gen, snap=snap).cpu()
    return out.half() if half else out


def parse_args(argv=None):
    """The command line; --compact is checked against -size here, before any model is loaded."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.compact is not None:
        if args.compact < 4:
            p.error("--compact: an index needs at least 4 vectors")
        if args.compact > args.size:
            p.error("--compact must not exceed -size (the vectors it compacts)")
        if args.compact_iters < 1:
            p.error("--compact-iters must be at least 1")
    elif args.compact_snap:
        p.error("--compact-snap needs --compact")
    return args


def build_parser():
    p = argparse.ArgumentParser(description="extract index")
    p.add_argument("--dataset-cache", default="dataset_cache")
    p.add_argument("-encp", "--encoder-path", default="models/encoder.pt")
    p.add_argument("-size", default=2048, type=int)
    p.add_argument("-o", "--output", default="models/index.pt")
    p.add_argument("-d", "--device", default="cuda")
    p.add_argument("--stride", default=4, type=int)
    p.add_argument("--seed", default=None, type=int, help="fix the shuffle (the reference does not seed it)")
    p.add_argument("--half", action="store_true", help="store the index in half precision (matched with the fp16 index storage: 2 B per element)")
    p.add_argument("--batch-frames", default=0, type=int,
                   help="encode the clips in ragged calls of at most this many frames and select the index on the device (0: clip by clip)")
    p.add_argument("--force-dist", action="store_true", help="run the WORLD_SIZE > 1 path (header-derived prefix, split, RCCL gather) even at world size 1")
    p.add_argument("--compact", default=None, type=int, metavar="K", help="compact the index of -size vectors to K k-means centroids on the device")
    p.add_argument("--compact-iters", default=8, type=int, help="k-means rounds of --compact")
    p.add_argument("--compact-snap", action="store_true", help="replace every centroid of --compact by its nearest real frame")
    return p


def main(argv=None):
    args = parse_args(argv)

    build_half = args.half and args.compact is None      # --compact works on the fp32 vectors; --half casts its result
    world, rank, local_rank = parallel.dist_env()
    sharded = world > 1 or args.force_dist
    device = torch.device(args.device)
    if sharded and device.type == "cuda" and device.index is None:
        device = torch.device("cuda", local_rank)
    if device.type == "cuda" and device.index is not None:
        torch.cuda.set_device(device)
    enc = Encoder()
    enc.load_state_dict(torch.load(args.encoder_path, map_location="cpu"))
    enc = enc.eval().to(device)
    files = sorted(glob.glob(os.path.join(args.dataset_cache, "*.wav")))
    if not files:
        sys.exit(f"no *.wav under {args.dataset_cache}")

    if not sharded:
        gen = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
        order = torch.randperm(len(files), generator=gen).tolist()      # DataLoader(shuffle=True) in the reference
        f0s = []
        if args.batch_frames > 0:
            tgt = batched_index(enc, device, files, order, args.stride, args.size, gen, build_half, args.batch_frames, f0s)
        else:
            feats, total = [], 0
            for i in order:
                z = encode_clip(enc, device, files[i], args.stride, f0s)
                feats.append(z)
                total += z.shape[2]
                if total > args.size:
                    break
            tgt = assemble(feats, args.size, gen, build_half)
        register = register_of(f0s)
    else:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        own_port = "MASTER_PORT" not in os.environ
        if own_port:                                                     # --force-dist without a launcher
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        own_group = not dist.is_initialized()
        if own_group:
            dist.init_process_group("nccl" if device.type == "cuda" else "gloo", rank=rank, world_size=world,
                                    **({"device_id": device} if device.type == "cuda" else {}))
        try:
            seed = torch.tensor([args.seed if args.seed is not None else int(torch.seed() & 0x7FFFFFFF)], dtype=torch.int64, device=device)
            dist.broadcast(seed, src=0)                                  # an unseeded run: rank 0's draw is everybody's
            gen = torch.Generator().manual_seed(int(seed.item()))
            order = torch.randperm(len(files), generator=gen).tolist()
            eng = enc.engine(device) if device.type == "cuda" else None
            cols = [clip_columns(f, args.stride, eng) for f in files]
            f0s = []
            feats = sharded_features(cols, order, args.size, world, rank, lambda i: encode_clip(enc, device, files[i], args.stride, f0s), device)
            tgt = assemble(feats, args.size, gen, build_half) if rank == 0 else None
            register = gathered_register(f0s, world, rank, device) if device.type == "cuda" else None
            dist.barrier()
        finally:
            if own_group:
                dist.destroy_process_group()
            if own_port:
                os.environ.pop("MASTER_PORT", None)
        if rank != 0:
            return 0
    if args.compact is not None:
        tgt = compacted(tgt, device, args.compact, args.compact_iters, args.compact_snap, gen, args.half)
    print(f"Extracted {tgt.shape[2]} vectors")
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    torch.save(tgt, args.output)
    if register is not None:
        save_register(args.output, register)
        print(f"Pitch register {float(register.median_hz[0]):.1f} Hz over {int(register.voiced[0])} voiced frames -> {sidecar_path(args.output)}")
    else:
        print(f"The clips' f0 could not be gathered on rank 0: no {sidecar_path(args.output)} written")
    return 0


if __name__ == "__main__":
    sys.exit(main())
