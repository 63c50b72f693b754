"""Edge cases and full-size properties of the HIP path (MI355X): shortest legal inputs, odd frame
counts, a long utterance with a large index, and size-independent invariants at the bench size."""
import pytest
import torch

from helpers import oracle_one_thread, rms, state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.mark.parametrize("frames,batch", [(3, 1), (4, 2), (5, 1), (7, 3), (33, 2), (61, 1)])
def test_short_and_odd_lengths_match_oracle(gen, frames, batch):
    """torch.stft's reflect padding needs L > 960, so T = 3 (1440 samples) is the shortest legal input."""
    enc_sd, dec_sd = state_dicts(0)
    L = frames * 480 - 17                       # ragged: autopad brings it back to frames * 480
    wf = synth.synth_wave(batch, L, seed=300 + frames)
    tgt = synth.synth_index(97, seed=frames)
    angle = synth.synth_angle(batch, frames, 70 + frames)
    with oracle_one_thread():
        ref = R.convert(enc_sd, dec_sd, wf, tgt, 0.5, angle)
    out = gen.convert(wf.to(DEV), tgt.to(DEV), 0.5, noise_angle=angle.to(DEV))
    assert out.shape == ref.shape == (batch, frames * 480)
    d = rms(out.cpu() - ref)
    print(f"[edge] T={frames} B={batch}: rms diff {d:.3e}")
    assert d <= 1e-4


def test_too_short_input_is_rejected_like_torch_stft(gen):
    from tinyvc_amd._lib import TinyVCError
    with pytest.raises(TinyVCError):
        gen.convert(torch.zeros(1, 960, device=DEV), synth.synth_index(16, seed=1).to(DEV), 0.0)


def test_long_utterance_large_index(gen):
    """20 s utterance (T = 1000) against a 20 000-vector index: staged comparison with the oracle.
    The waveform gate is looser here: 1000 frames of f0 integrate fp32-ulp differences into phase."""
    enc_sd, dec_sd = state_dicts(0)
    wf = synth.synth_wave(1, 480000, seed=900)
    tgt = synth.synth_index(20000, seed=901)
    angle = synth.synth_angle(1, 1000, 902)
    st = R.convert(enc_sd, dec_sd, wf, tgt, 0.0, angle, return_stages=True)
    from tinyvc_amd.module import utils
    from tinyvc_amd.module.tinyvc import match_features
    w = wf.to(DEV)
    spec = utils.spectrogram(w)
    assert rms(spec.cpu() - st["spec"]) / rms(st["spec"]) < 2e-6
    ssl, f0 = gen.encoder.infer(spec)
    assert rms(ssl.cpu() - st["ssl"]) / rms(st["ssl"]) < 2e-5
    m, idx = match_features(st["ssl"].to(DEV), tgt.to(DEV), return_indices=True)
    _o, oidx, sims = R.match_features(st["ssl"], tgt, return_indices=True)
    top = torch.topk(sims.double(), 5, dim=2).values
    decidable = (top[..., :-1] - top[..., 1:]).min(dim=2).values > 1e-5
    assert decidable.float().mean() > 0.9
    assert torch.equal(idx.cpu()[decidable], oidx[decidable])
    wave = gen.decoder.infer(st["matched"].to(DEV), st["f0s"].to(DEV), st["energy"].to(DEV), noise_angle=angle.to(DEV))
    d = rms(wave.cpu() - st["wave"])
    print(f"[edge] 20 s decoder (oracle inputs): rms diff {d:.3e}")
    assert d <= 1e-5
    full = gen.convert(w, tgt.to(DEV), 0.0, noise_angle=angle.to(DEV))
    d2 = rms(full.cpu() - st["wave"])
    print(f"[edge] 20 s end to end: rms diff {d2:.3e}")
    assert d2 <= 5e-4      # measured 1.8e-4; no discrete failure (phase slip, flipped neighbour); the arithmetic claim at this length is test_gpu_truth.py (T = 1000)


def test_full_bench_size_properties(gen):
    """BASELINE configs[1] size (64 x 4 s, 10 k index): invariants that need no oracle run."""
    wf = synth.synth_wave(64, 96000, seed=100).to(DEV)
    tgt = synth.synth_index(10000, seed=4).to(DEV)
    angle = synth.synth_angle(64, 200, 5).to(DEV)
    out = gen.convert(wf, tgt, 0.0, noise_angle=angle)
    assert out.shape == (64, 96000) and torch.isfinite(out).all()
    again = gen.convert(wf, tgt, 0.0, noise_angle=angle)
    assert torch.equal(out, again)                                     # idempotent / deterministic
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).to(DEV)
    outp = gen.convert(wf[perm], tgt, 0.0, noise_angle=angle[perm])
    assert torch.equal(outp, out[perm])                                # utterances do not interact
    sub = gen.convert(wf[5:9], tgt, 0.0, noise_angle=angle[5:9])
    assert torch.equal(sub, out[5:9])                                  # batch-size invariant
    # kNN self-consistency at size: every index vector's nearest neighbour in the index is itself
    from tinyvc_amd.module.tinyvc import match_features
    q = tgt[:, :, :512].contiguous()
    _m, idx = match_features(q, tgt, return_indices=True)
    assert torch.equal(idx[0, :, 0].cpu(), torch.arange(512))


def test_thirty_two_concurrent_streams(gen):
    """BASELINE configs[2]: 32 streams through one batched convert + one SOLA launch per block (HIP-graph replay).  Every
    stream must equal the same stream run alone (streams do not interact), and a block must fit the 80 ms real-time budget."""
    import time
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    S, nblk = 32, 6
    tgt = synth.synth_index(1000, seed=2).to(DEV)
    blocks = torch.stack([synth.synth_wave(1, nblk * 1920, seed=200 + s)[0] for s in range(S)]).view(S, nblk, 1920).to(DEV)
    st = BatchedStreamInfer(gen, n_streams=S, target=tgt, device=torch.device(DEV), block_size=1920, extra_size=3840, use_graph=True)
    st.init_buffer()
    outs, lat = [], []
    for i in range(nblk):
        angle = synth.synth_angle(S, st.input_size // 480, 900 + i).to(DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs.append(st.audio_callback(blocks[:, i], noise_angle=angle).clone())
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
    outs = torch.stack(outs, 1)                       # [S, nblk, 1920]
    assert torch.isfinite(outs).all()
    print(f"[edge] 32 streams: block latencies (ms) {[round(x, 2) for x in lat]}")
    assert min(lat[3:]) < 80.0
    for s in (0, 13, 31):                             # the same stream alone, eager, same phases
        one = StreamInfer(gen, target=tgt, device=torch.device(DEV), block_size=1920, extra_size=3840)
        one.init_buffer()
        for i in range(nblk):
            angle = synth.synth_angle(S, st.input_size // 480, 900 + i)[s:s + 1].to(DEV)
            o = one.audio_callback(blocks[s, i], noise_angle=angle)
            assert torch.equal(o, outs[s, i]), f"stream {s} block {i}: batched != alone"


@pytest.mark.parametrize("n_index", [4, 129, 1001, 10000])
def test_fp16_index_storage_matches_oracle_on_the_rounded_vectors(gen, n_index):
    """An index handed over as torch.float16 takes the fp16 storage (2 B per element).  Its results must equal the
    reference's on the SAME fp16-rounded vectors: indices wherever fp32 can decide, and the mean of the four rows."""
    from tinyvc_amd.module.tinyvc import match_features
    g = torch.Generator().manual_seed(n_index)
    index16 = torch.randn(1, 768, n_index, generator=g).half()
    src = torch.randn(2, 768, 37, generator=g)
    out, idx = match_features(src.to(DEV), index16.to(DEV), return_indices=True)
    o_out, o_idx, sims = R.match_features(src, index16.float(), return_indices=True)
    top = torch.topk(sims.double(), min(5, n_index), dim=2).values
    decidable = (top[..., :-1] - top[..., 1:]).min(dim=2).values > 1e-5
    assert decidable.float().mean() > 0.9
    assert torch.equal(idx.cpu()[decidable], o_idx[decidable])
    assert (idx.cpu() < n_index).all() and (idx.cpu() >= 0).all()
    m = decidable[:, None, :].expand_as(o_out)
    assert torch.equal(out.cpu()[m], o_out[m]), "mean of the four fp16 rows must be bit-identical once the indices are"
    # and the fp32 storage on the rounded vectors selects the same rows
    _o32, idx32 = match_features(src.to(DEV), index16.float().to(DEV), return_indices=True)
    assert torch.equal(idx32.cpu()[decidable], idx.cpu()[decidable])


def test_cfg5_five_minutes_against_a_million_vector_fp16_index(gen):
    """BASELINE configs[4]: one 5-minute utterance (T = 15 000 frames), 1 000 000-vector index in fp16 storage.
    The reference cannot run this size (its sims tensor would be 60 GB), so: (1) the kNN stage against the oracle on a
    200-query slice; (2) fp16 storage vs fp32 storage on all 15 000 queries (mismatches only at near-ties); (3) the
    workspace the library asks for; (4) the whole conversion, finite, timed, with the kNN stage's matrix-pipe fraction."""
    import ctypes
    import time
    from tinyvc_amd.module import utils
    from tinyvc_amd.module.tinyvc import match_features
    eng = gen.engine(DEV)
    T, N = 15000, 1_000_000
    wf = synth.synth_wave(1, 480 * T, seed=6)
    index16 = synth.synth_index(N, seed=7).half()                 # [1, 768, N] fp16: 1.5 GB
    ssl, _f0 = gen.encode(wf.to(DEV))
    d16 = index16.to(DEV)
    blob16, n = eng.knn_prepare(d16)
    assert blob16.numel() * 4 < 1.55e9, "fp16 storage must be 2 B per element"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sims16, idx16 = eng.knn_topk(ssl, blob16, n)
    torch.cuda.synchronize()
    t_knn = time.perf_counter() - t0
    print(f"[cfg5] kNN T={T} x N={N}: {t_knn * 1e3:.1f} ms = {T * N / t_knn / 1e9:.0f} G (query, vector) pairs/s "
          f"(two-stage search: one fp16 product per pair in the coarse passes = {1.125 * 2 * 768 * T * N / t_knn / 2.5e15:.2f} of the f16 MFMA peak, "
          f"then an exact fp32 rescoring of a few dozen candidates per query; the exact kernel alone needs ~137 ms)")
    # (1) oracle on a 200-query slice, on the same fp16-rounded vectors
    q = ssl[:, :, 7000:7200].cpu()
    ref = index16.float()
    _o, o_idx, sims = R.match_features(q, ref, return_indices=True)
    top = torch.topk(sims, 5, dim=2).values
    decidable = (top[..., :-1] - top[..., 1:]).min(dim=2).values > 1e-5
    got = idx16[:, 7000:7200].cpu()
    print(f"[cfg5] oracle slice: {int(decidable.sum())} of 200 queries decidable at 1e-5; all equal: {torch.equal(got[decidable], o_idx[decidable])}")
    assert decidable.float().mean() > 0.5 and torch.equal(got[decidable], o_idx[decidable])
    del sims, top, _o
    # (2) fp32 storage of the same vectors, all queries (split-N merge at this size: 9 index splits x 118 query tiles)
    d32 = ref.to(DEV)
    del ref
    blob32, _ = eng.knn_prepare(d32)
    sims32, idx32 = eng.knn_topk(ssl, blob32, n)
    differ = (idx32 != idx16).any(dim=2)
    gap = (sims32[..., :-1] - sims32[..., 1:]).abs().min(dim=2).values
    rate = float(differ.float().mean())
    print(f"[cfg5] fp16 vs fp32 storage: {int(differ.sum())} of {T} queries differ ({rate * 100:.3f} %); largest top-4 gap among them "
          f"{float(gap[differ].max()) if differ.any() else 0.0:.2e}; similarity rms diff {float((sims32 - sims16).pow(2).mean().sqrt()):.2e}")
    assert rate < 0.01
    assert not differ.any() or float(gap[differ].max()) < 1e-5, "a mismatch away from a near-tie"
    del blob32, d32, sims32, idx32
    # (3) the workspace for the whole conversion at this size
    need = ctypes.c_size_t()
    assert eng.lib.tvc_workspace_bytes(eng.ctx, 1, 480 * T, N, ctypes.byref(need)) == 0
    print(f"[cfg5] tvc_workspace_bytes(B=1, L={480 * T}, N={N}) = {need.value / 2**30:.2f} GiB")
    assert need.value < 32 * 2**30
    # (4) the whole path, one call
    eng.profile(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = gen.convert(wf.to(DEV), d16, 0.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof = eng.profile_read()
    eng.profile(False)
    assert out.shape == (1, 480 * T) and torch.isfinite(out).all()
    print(f"[cfg5] 5-minute convert: {dt * 1e3:.0f} ms wall ({300 / dt:.0f}x real time); stages (ms): "
          + ", ".join(f"{k} {v:.1f}" for k, v in sorted(prof.items()) if not k.startswith("filter.")))
    # the staged kNN equals what convert used: same rows for the slice
    m16, _ = match_features(ssl[:, :, 7000:7200].contiguous(), d16, return_indices=True)
    assert torch.isfinite(m16).all()


def test_noise_angle_map_equals_the_reference_expression():
    """decoder.py:78 draws `torch.rand(...) * 2 * math.pi - math.pi` (three tensor ops); the module path applies them as ONE launch
    (tvc_noise_angle_from_uniform_f32): bit-identical, odd sizes and the ends of the interval included, and the draw is torch's own."""
    import math
    from tinyvc_amd.engine import default_engine
    from tinyvc_amd.module.tinyvc import Decoder
    eng = default_engine(torch.device(DEV))
    for n in (1, 3, 4, 5, 1023, 961 * 200 + 7):
        u = torch.rand(n + 1, device=DEV)[1:].contiguous()          # (a 4-byte-aligned start: the vector path must not assume 16)
        u[0] = 0.0
        u[-1] = 1.0 - 2.0 ** -24
        want = u * 2 * math.pi - math.pi
        got = eng.noise_angle_from_uniform(u.clone())
        assert torch.equal(got, want), n
    torch.manual_seed(1234)
    a = Decoder.draw_noise_angle(3, 17, torch.device(DEV))
    torch.manual_seed(1234)
    b = torch.rand(3, 961, 17, device=DEV) * 2 * math.pi - math.pi
    assert torch.equal(a, b)


def test_seeded_draw_is_refused_inside_a_stream_capture_and_push_equals_roll(gen):
    """C-ABI rules of round 6.  (1) noise_angle = NULL makes the seed a kernel argument, which a capture would bake into the graph - every
    replay the same noise -: the call is refused with TVC_ERR_STATE while the stream is capturing, launches nothing, and the same call with
    phases passes.  (2) tvc_stream_push_f32 is stream.py:69-70's roll + slice assignment, bit for bit."""
    from tinyvc_amd.engine import _ptr
    eng = gen.engine(DEV)
    B, T = 2, 12
    f0 = (torch.rand(B, 1, T, device=DEV) * 200 + 80).contiguous()
    amps = torch.rand(B, 15, T, device=DEV).contiguous()
    kern = torch.rand(B, 961, T, device=DEV).contiguous()
    angle = synth.synth_angle(B, T, 4).to(DEV)
    src = torch.zeros(B, 16, T * 480, device=DEV)
    eager = eng.dsp(f0, amps, kern, noise_angle=angle)
    p, n = eng._wsargs(B, T * 480)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = eng._stream()
        rc_null = eng.lib.tvc_dsp_f32(eng.ctx, s, _ptr(f0), _ptr(amps), _ptr(kern), None, 123, _ptr(src), B, T, p, n)
        rc_ok = eng.lib.tvc_dsp_f32(eng.ctx, s, _ptr(f0), _ptr(amps), _ptr(kern), _ptr(angle), 0, _ptr(src), B, T, p, n)
    assert rc_null == -3, (rc_null, eng.lib.tvc_last_error(eng.ctx))            # TVC_ERR_STATE
    assert rc_ok == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(src, eager), "the captured call with injected phases replays the eager result"

    buf = torch.randn(5, 13440, device=DEV)
    blk = torch.randn(5, 1920, device=DEV)
    want = torch.roll(buf, -1920, dims=1)
    want[:, -1920:] = blk
    got = eng.stream_push(buf.clone(), blk)
    assert torch.equal(got, want)
    odd = torch.randn(3, 2000, device=DEV)                     # a buffer that is not a multiple of the workgroup, block = almost all of it
    b2 = torch.randn(3, 1999, device=DEV)
    w2 = torch.cat([odd[:, 1999:], b2], dim=1)
    assert torch.equal(eng.stream_push(odd.clone(), b2), w2)


@pytest.mark.parametrize("n", [32768, 32769, 48000, 120000])
def test_stream_push_equals_roll_past_32768_samples(gen, n):
    """tvc_stream_push_f32 on stream buffers of any length: infer.py --chunked -c 9600 rolls a 48 000-sample buffer, infer_streaming.py
    -c 24000 one of 35 520.  A row longer than 32 768 samples is shifted tile by tile inside the one launch; bit for bit stream.py:69-70's
    roll + slice assignment, for one and for three streams, blocks from 1920 samples to all but one sample of the buffer."""
    eng = gen.engine(DEV)
    g = torch.Generator().manual_seed(n)
    for S in (1, 3):
        for m in (1920, 9600, n - 1):
            buf = torch.randn(S, n, generator=g).to(DEV)
            blk = torch.randn(S, m, generator=g).to(DEV)
            want = torch.roll(buf, -m, dims=1)
            want[:, -m:] = blk
            got = eng.stream_push(buf.clone(), blk)
            assert torch.equal(got, want), (S, n, m)


def test_workspace_of_exactly_the_measured_peak_and_one_byte_less(gen):
    """Every entry measures its workspace with a walk that launches nothing (ws.dry) before its launching walk, and checks behind the second
    that it took no more (api.h run_walks).  tvc_workspace_bytes - 4096 is that peak: a conversion in exactly it equals one in the engine's
    own workspace bit for bit, and one byte less is refused with TVC_ERR_WORKSPACE before anything launches (the output keeps its NaN fill).
    The same for a ragged call with tvc_workspace_bytes_ragged - 4096."""
    import ctypes
    from tinyvc_amd.engine import _ptr
    eng = gen.engine(DEV)
    B, T = 2, 40
    L = 480 * T
    wf = synth.synth_wave(B, L, seed=41).to(DEV)
    blob, n = eng.knn_prepare(synth.synth_index(300, seed=42).to(DEV))
    angle = synth.synth_angle(B, T, 43).to(DEV)
    want = eng.convert(wf, blob, n, 0.5, noise_angle=angle)
    need = ctypes.c_size_t()
    assert eng.lib.tvc_workspace_bytes(eng.ctx, B, L, n, ctypes.byref(need)) == 0
    for extra, rc_want in ((0, 0), (-1, -4)):                          # -4: TVC_ERR_WORKSPACE
        ws = torch.empty(need.value - 4096 + extra, dtype=torch.uint8, device=DEV)
        out = torch.full((B, L), float("nan"), device=DEV)
        rc = eng.lib.tvc_convert_f32(eng.ctx, eng._stream(), _ptr(wf), _ptr(blob), n, 0.5, _ptr(angle), 0, _ptr(out), B, L, _ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert rc == rc_want, (extra, rc, eng.lib.tvc_last_error(eng.ctx))
        if rc == 0:
            assert torch.equal(out, want), "a conversion in exactly the measured workspace"
        else:
            assert out.isnan().all(), "a refused call launched something"

    frames = [40, 13, 7]
    lens = (ctypes.c_int64 * 3)(*[480 * f for f in frames])
    wr = torch.zeros(3, L, device=DEV)
    for b, f in enumerate(frames):
        wr[b, :480 * f] = wf[b % B, :480 * f]
    ar = synth.synth_angle(3, T, 44).to(DEV)
    assert eng.lib.tvc_workspace_bytes_ragged(eng.ctx, 3, L, lens, n, ctypes.byref(need)) == 0
    for extra, rc_want in ((0, 0), (-1, -4)):
        ws = torch.empty(need.value - 4096 + extra, dtype=torch.uint8, device=DEV)
        out = torch.full((3, L), float("nan"), device=DEV)
        rc = eng.lib.tvc_convert_ragged_f32(eng.ctx, eng._stream(), _ptr(wr), L, lens, _ptr(blob), n, 0.5, _ptr(ar), 0, _ptr(out), 3, _ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert rc == rc_want, (extra, rc, eng.lib.tvc_last_error(eng.ctx))
        if rc == 0:
            assert torch.equal(out, eng.convert_ragged(wr, [480 * f for f in frames], blob, n, 0.5, noise_angle=ar)), "a ragged call in exactly the measured workspace"
        else:
            assert out.isnan().all(), "a refused ragged call launched something"


def test_exact_workspace_for_the_multi_ragged_encode_and_compact_entries(gen):
    """The contract of the test above - a call in exactly the measured peak equals the engine's own call bit for bit, one byte less is
    refused with TVC_ERR_WORKSPACE before anything launches (every output keeps its fill: NaN, or -7 in the integer tensors) - for the
    other entries that walk twice: tvc_convert_multi_f32, tvc_knn_match_multi_f32, tvc_convert_ragged_multi_f32, tvc_encode_ragged_f32
    (several batches, so the packing launch too) and tvc_index_compact_f32 (assign_out = NULL: the call its query measures).  The peak is the entry's tvc_workspace_bytes* - 4096;
    tvc_knn_match_multi_f32 has no query of its own (the engine gives it a conversion's workspace), so its peak is read from the
    refusal of a call without any workspace ("need <peak> bytes")."""
    import ctypes
    import re
    from tinyvc_amd.engine import _ptr
    eng = gen.engine(DEV)
    lib, ctx = eng.lib, eng.ctx
    nan = float("nan")

    def exact_and_one_less(what, peak, fresh, call, check):
        """call(outs, ws, nbytes) -> rc at `peak` bytes (then check(outs)) and at peak - 1 (then every out keeps its fill)"""
        for extra, rc_want in ((0, 0), (-1, -4)):                      # -4: TVC_ERR_WORKSPACE
            ws = torch.empty(peak + extra, dtype=torch.uint8, device=DEV)
            outs = fresh()
            rc = call(outs, _ptr(ws), ws.numel())
            torch.cuda.synchronize()
            assert rc == rc_want, (what, extra, rc, lib.tvc_last_error(ctx))
            if rc == 0:
                check(outs)
            else:
                for o in outs:
                    assert (o.isnan() if o.is_floating_point() else o == -7).all(), f"{what}: a refused call launched something"

    B, T = 2, 40
    L = 480 * T
    wf = synth.synth_wave(B, L, seed=51).to(DEV)
    b1, n1 = eng.knn_prepare(synth.synth_index(300, seed=52).to(DEV))
    b2, n2 = eng.knn_prepare(synth.synth_index(260, seed=53).to(DEV))
    need = ctypes.c_size_t()

    # ---- tvc_convert_multi_f32: two rows, two indices, one shift per row
    blobs, ns, sh = (ctypes.c_void_p * 2)(b1.data_ptr(), b2.data_ptr()), (ctypes.c_int64 * 2)(n1, n2), (ctypes.c_float * 2)(0.5, -1.0)
    angle = synth.synth_angle(B, T, 54).to(DEV)
    want = eng.convert_multi(wf, [b1, b2], [n1, n2], [0.5, -1.0], noise_angle=angle)
    assert lib.tvc_workspace_bytes_multi(ctx, B, L, ns, ctypes.byref(need)) == 0
    multi_bytes = need.value

    def check_wave(outs):
        assert torch.equal(outs[0], want)
    exact_and_one_less("convert_multi", multi_bytes - 4096, lambda: [torch.full((B, L), nan, device=DEV)],
                       lambda o, p, nb: lib.tvc_convert_multi_f32(ctx, eng._stream(), _ptr(wf), blobs, ns, 0.0, sh, _ptr(angle), 0, _ptr(o[0]), B, L, p, nb), check_wave)

    # ---- tvc_knn_match_multi_f32: the same table, indices wanted
    src = torch.randn(B, 768, T, generator=torch.Generator().manual_seed(55)).to(DEV)
    want_m, want_i = eng.knn_match_multi(src, [b1, b2], [n1, n2], want_indices=True)

    def match(o, p, nb):
        return lib.tvc_knn_match_multi_f32(ctx, eng._stream(), _ptr(src), blobs, ns, _ptr(o[0]), _ptr(o[1]), B, T, p, nb)
    probe = [torch.full((B, 768, T), nan, device=DEV), torch.full((B, T, 4), -7, dtype=torch.int64, device=DEV)]
    assert match(probe, None, 0) == -4
    peak = int(re.search(rb"need (\d+) bytes", lib.tvc_last_error(ctx)).group(1))
    assert 0 < peak <= multi_bytes - 4096, "the engine's workspace for this call covers it"

    def check_match(outs):
        assert torch.equal(outs[0], want_m) and torch.equal(outs[1], want_i)
    exact_and_one_less("knn_match_multi", peak, lambda: [torch.full((B, 768, T), nan, device=DEV), torch.full((B, T, 4), -7, dtype=torch.int64, device=DEV)],
                       match, check_match)

    # ---- tvc_convert_ragged_multi_f32: two length classes = two batches; rows 0 and 2 share an index
    frames = [40, 13, 7]
    lengths = [480 * f for f in frames]
    lens = (ctypes.c_int64 * 3)(*lengths)
    wr = torch.zeros(3, L, device=DEV)
    for b, f in enumerate(frames):
        wr[b, :480 * f] = wf[b % B, :480 * f]
    blobs3, ns3, sh3 = (ctypes.c_void_p * 3)(b1.data_ptr(), b2.data_ptr(), b1.data_ptr()), (ctypes.c_int64 * 3)(n1, n2, n1), (ctypes.c_float * 3)(0.5, -1.0, 2.0)
    ar = synth.synth_angle(3, T, 56).to(DEV)
    want_r = eng.convert_ragged_multi(wr, lengths, [b1, b2, b1], [n1, n2, n1], [0.5, -1.0, 2.0], noise_angle=ar)
    assert lib.tvc_workspace_bytes_ragged_multi(ctx, 3, L, lens, ns3, ctypes.byref(need)) == 0

    def check_ragged(outs):
        assert torch.equal(outs[0], want_r)
    exact_and_one_less("convert_ragged_multi", need.value - 4096, lambda: [torch.full((3, L), nan, device=DEV)],
                       lambda o, p, nb: lib.tvc_convert_ragged_multi_f32(ctx, eng._stream(), _ptr(wr), L, lens, blobs3, ns3, 0.0, sh3, _ptr(ar), 0, _ptr(o[0]), 3, p, nb),
                       check_ragged)

    # ---- tvc_encode_ragged_f32 under a cap of 45 frames: batches [40] and [13, 7], packed by pack_batch_kernel
    S = sum(frames)
    try:
        eng.set_ragged_batch_frames(45)
        want_ssl, want_f0, _ = eng.encode_ragged(wr, lengths)
        assert lib.tvc_workspace_bytes_encode_ragged(ctx, 3, L, lens, ctypes.byref(need)) == 0

        def check_enc(outs):
            assert torch.equal(outs[0], want_ssl) and torch.equal(outs[1], want_f0)
        exact_and_one_less("encode_ragged", need.value - 4096, lambda: [torch.full((768, S), nan, device=DEV), torch.full((S,), nan, device=DEV)],
                           lambda o, p, nb: lib.tvc_encode_ragged_f32(ctx, eng._stream(), _ptr(wr), L, lens, _ptr(o[0]), _ptr(o[1]), 3, p, nb), check_enc)
    finally:
        eng.set_ragged_batch_frames(0)

    # ---- tvc_index_compact_f32: 300 points -> 8 centroids, two rounds; the accepted call records its blob for N = K
    N, K, iters = n1, 8, 2
    cols = (torch.arange(K, dtype=torch.int64) * 37).to(DEV)
    w_index, w_blob, w_assign, w_counts, w_moved = eng.index_compact(b1, N, cols, iters)
    q = src[:1].contiguous()
    w_top = eng.knn_topk(q, w_blob, K)
    assert lib.tvc_workspace_bytes_index_compact(ctx, N, K, ctypes.byref(need)) == 0

    def fresh_compact():
        return [torch.full((1, 768, K), nan, device=DEV), eng._owned(torch.full((lib.tvc_knn_prepared_elems(K),), nan, device=DEV)),
                torch.full((K,), -7, dtype=torch.int32, device=DEV), torch.full((iters,), -7, dtype=torch.int32, device=DEV)]

    def check_compact(outs):
        index, blob, counts, moved = outs
        assert torch.equal(index, w_index) and torch.equal(counts, w_counts) and torch.equal(moved, w_moved)
        assert int(counts.sum()) == N and torch.equal(torch.bincount(w_assign, minlength=K).int(), counts)
        top = eng.knn_topk(q, blob, K)                                 # (the blob's unwritten padding is whatever the buffer held: compared through a search)
        assert torch.equal(top[0], w_top[0]) and torch.equal(top[1], w_top[1])
    # assign_out = NULL: the assignment then lives in the workspace, which is the call the query measures (with assign_out it needs N * 8 bytes less)
    exact_and_one_less("index_compact", need.value - 4096, fresh_compact,
                       lambda o, p, nb: lib.tvc_index_compact_f32(ctx, eng._stream(), _ptr(b1), N, _ptr(cols), K, iters, _ptr(o[0]), _ptr(o[1]), None, _ptr(o[2]),
                                                                  _ptr(o[3]), p, nb), check_compact)
