"""One speaker index per utterance and per stream (tvc_knn_match_multi_f32, tvc_convert_multi_f32, tvc_convert_ragged_multi_f32).

The reference's match_features takes reference [B, 768, N] and matches row b against reference[b] (a bmm over the batch,
feature_retrieval.py:15-33).  Contract here: every row of a multi-index call is bit-identical to its own B = 1 call against its own
blob - the kNN stage, the whole conversion (equal and ragged batches, per-row pitch shifts) and the batched stream."""
import ctypes

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


@pytest.fixture(scope="module")
def targets():
    """Four distinct indices: the exact kernel (N = 300), the two-stage search (6 000), fp16 storage (12 000), another 6 000."""
    return [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV),
            synth.synth_index(12000, seed=23).half().to(DEV), synth.synth_index(6000, seed=24).to(DEV)]


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def test_knn_multi_rows_equal_their_own_calls_and_the_oracle(targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    B, T = 4, 333                                            # partial query tiles in every segment
    g = torch.Generator().manual_seed(5)
    src = torch.randn(B, 768, T, generator=g)
    blobs, ns = prepare_references(targets)
    out, idx = eng.knn_match_multi(src.to(DEV), blobs, ns, want_indices=True)
    for b in range(B):
        o1, i1 = eng.knn_match(src[b:b + 1].to(DEV), blobs[b], ns[b], want_indices=True)
        assert torch.equal(idx[b:b + 1], i1), f"row {b}: indices differ from its B = 1 call"
        assert torch.equal(out[b:b + 1], o1), f"row {b}: matched features differ from its B = 1 call"
        # the oracle (fp16 row: on the same fp16-rounded vectors) wherever fp32 can decide the top 4
        ref = targets[b].float().cpu()
        r_out, r_idx, sims = R.match_features(src[b:b + 1], ref, return_indices=True)
        top = torch.topk(sims, 5, dim=2).values
        ok = (top[..., :-1] - top[..., 1:]).min(dim=2).values > 1e-5
        assert ok.float().mean() > 0.9
        assert torch.equal(idx[b].cpu()[ok[0]], r_idx[0][ok[0]]), f"row {b}: indices differ from the oracle on decidable columns"


def test_knn_multi_overflow_falls_back_per_segment():
    """A dense neighbourhood overflows the candidate lists of one segment: only that segment takes the exact kernel, and every row
    still equals its own call."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    T = 100
    g = torch.Generator().manual_seed(9)
    src = torch.randn(3, 768, T, generator=g)
    dense = torch.randn(1, 768, 5000, generator=g)
    dense[0, :, :400] = src[1, :, :1] + 1e-4 * torch.randn(768, 400, generator=g)      # 400 near-copies of row 1's first query
    tg = [synth.synth_index(5000, seed=31).to(DEV), dense.to(DEV), synth.synth_index(5000, seed=32).to(DEV)]
    blobs, ns = prepare_references(tg)
    out, idx = eng.knn_match_multi(src.to(DEV), blobs, ns, want_indices=True)
    for b in range(3):
        o1, i1 = eng.knn_match(src[b:b + 1].to(DEV), blobs[b], ns[b], want_indices=True)
        assert torch.equal(idx[b:b + 1], i1) and torch.equal(out[b:b + 1], o1), f"row {b}"
    assert int(idx[1, 0].max()) < 400


def test_convert_equal_lengths_rows_equal_their_own_calls(gen, targets):
    enc_sd, dec_sd = state_dicts(0)
    B, T = 4, 200
    wf = synth.synth_wave(B, T * 480, seed=41)
    angle = synth.synth_angle(B, T, 42).to(DEV)
    out = gen.convert(wf.to(DEV), targets, 0.5, noise_angle=angle)
    worst = 0.0
    for b in range(B):
        one = gen.convert(wf[b:b + 1].to(DEV), targets[b], 0.5, noise_angle=angle[b:b + 1].contiguous())
        assert torch.equal(out[b:b + 1], one), f"row {b}: multi-index convert != its B = 1 call"
        with oracle_one_thread():
            ref = R.convert(enc_sd, dec_sd, wf[b:b + 1], targets[b].float().cpu(), 0.5, angle[b:b + 1].cpu())
        d = rms(out[b].cpu() - ref[0])
        worst = max(worst, d)
        assert d <= 1e-4, f"row {b}: {d:.3e} rms vs the oracle"
    print(f"[multi] 4 rows against 4 indices: each equals its B = 1 call; worst rms vs the oracle {worst:.3e}")
    # every row given the same blob: one segment, today's single-index call bit for bit
    same = gen.convert(wf.to(DEV), [targets[1]] * B, 0.5, noise_angle=angle)
    shared = gen.convert(wf.to(DEV), targets[1], 0.5, noise_angle=angle)
    assert torch.equal(same, shared)
    # the reference's own form: one [B, 768, N] tensor
    stacked = torch.stack([synth.synth_index(700, seed=50 + b)[0] for b in range(B)]).to(DEV)
    out2 = gen.convert(wf.to(DEV), stacked, 0.5, noise_angle=angle)
    for b in (0, 3):
        one = gen.convert(wf[b:b + 1].to(DEV), stacked[b:b + 1].clone(), 0.5, noise_angle=angle[b:b + 1].contiguous())
        assert torch.equal(out2[b:b + 1], one)


def test_ragged_batch_with_one_index_per_row(gen, targets):
    """Lengths in all four length classes, a frame cap that cuts the classes into several in-kernel batches: every row equals its own
    B = 1 call against its own index.  (Before this feature the call raised: a ragged batch took one shared index.)"""
    frames = [7, 150, 33, 60, 9, 131, 20, 90]
    lens = [480 * f - (11 if i % 2 else 0) for i, f in enumerate(frames)]
    B, Lmax, Tmax = len(frames), 480 * max(frames), max(frames)
    wf = torch.zeros(B, Lmax)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=600 + b)[0]
    tg = [targets[b % 4] for b in range(B)]
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    eng = gen.engine()
    try:
        for cap in (0, 100):
            eng.set_ragged_batch_frames(cap)
            out = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens)
            for b, f in enumerate(frames):
                one = gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tg[b], -2.0, noise_angle=angle[b:b + 1, :, :f].contiguous())
                assert torch.equal(out[b, :480 * f], one[0]), f"cap {cap}, row {b} ({f} frames)"
                assert not out[b, 480 * f:].any()
    finally:
        eng.set_ragged_batch_frames(0)


def test_per_row_pitch_shift(gen, targets):
    shifts = [-12.0, 0.0, 7.0, 12.0]
    B, T = 4, 60
    wf = synth.synth_wave(B, T * 480, seed=71)
    angle = synth.synth_angle(B, T, 72).to(DEV)
    shared = targets[0]
    for tg in (targets, shared):                              # distinct indices, and one shared index with a shift per row
        out = gen.convert(wf.to(DEV), tg, torch.tensor(shifts), noise_angle=angle)
        for b in range(B):
            t = tg[b] if isinstance(tg, list) else tg
            one = gen.convert(wf[b:b + 1].to(DEV), t, shifts[b], noise_angle=angle[b:b + 1].contiguous())
            assert torch.equal(out[b:b + 1], one), f"row {b}, shift {shifts[b]}"
    frames = [40, 12, 60, 25]
    lens = [480 * f for f in frames]
    wr = torch.zeros(B, 480 * max(frames))
    for b, n in enumerate(lens):
        wr[b, :n] = wf[b, :n]
    out = gen.convert(wr.to(DEV), targets, shifts, noise_angle=angle, lengths=lens)
    for b, f in enumerate(frames):
        one = gen.convert(wr[b:b + 1, :lens[b]].to(DEV), targets[b], shifts[b], noise_angle=angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b, :480 * f], one[0]), f"ragged row {b}, shift {shifts[b]}"


def test_batched_streams_with_their_own_targets(gen, targets, monkeypatch):
    from tinyvc_amd.engine import Engine
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    S, nblk = 3, 6
    tg = [synth.synth_index(300, seed=81).to(DEV), synth.synth_index(5000, seed=82).to(DEV), synth.synth_index(800, seed=83).to(DEV)]
    shifts = [0.0, 3.0, -5.0]
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)
    calls = []
    real = Engine.knn_prepare
    monkeypatch.setattr(Engine, "knn_prepare", lambda self, index: calls.append(1) or real(self, index))
    outs = {}
    for use_graph in (False, True):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=shifts, device=torch.device(DEV), block_size=1920,
                                extra_size=3840, use_graph=use_graph)
        st.init_buffer()
        res = []
        for i in range(nblk):
            n0 = len(calls)
            angle = synth.synth_angle(S, st.input_size // 480, 850 + i).to(DEV)
            res.append(st.audio_callback(blocks[:, i], noise_angle=angle).clone())
            if i > 0 or use_graph:
                assert len(calls) == n0, f"block {i} prepared an index again"
        outs[use_graph] = torch.stack(res, 1)
        if use_graph:
            assert st._graph is not None and True in st._graph[1], "blocks 3.. must have replayed the captured graph"
    assert len(calls) == S
    assert torch.equal(outs[False], outs[True]), "graph replay != eager"
    for s in range(S):
        one = StreamInfer(gen, target=tg[s], pitch_shift=shifts[s], device=torch.device(DEV), block_size=1920, extra_size=3840)
        one.init_buffer()
        for i in range(nblk):
            angle = synth.synth_angle(S, one.input_size // 480, 850 + i)[s:s + 1].to(DEV)
            o = one.audio_callback(blocks[s, i], noise_angle=angle)
            assert torch.equal(o, outs[False][s, i]), f"stream {s} block {i}: batched != alone"


def test_bad_tables_are_refused_before_any_launch(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = gen.engine()
    lib = eng.lib
    blobs, ns = prepare_references(targets[:2])
    B, T = 2, 40
    src = torch.randn(B, 768, T, device=DEV)
    out = torch.full((B, 768, T), 7.0, device=DEV)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def call(ptrs, nvec):
        arr = (ctypes.c_void_p * B)(*ptrs)
        nn = (ctypes.c_int64 * B)(*nvec)
        return lib.tvc_knn_match_multi_f32(eng.ctx, eng._stream(), ctypes.c_void_p(src.data_ptr()), arr, nn, ctypes.c_void_p(out.data_ptr()),
                                           None, B, T, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel()))

    ptrs = [b.data_ptr() for b in blobs]
    assert call([ptrs[0], None], ns) == -1                        # a null blob
    assert call(ptrs, [ns[0], 3]) == -1                           # N < 4
    assert call(ptrs, [ns[0], ns[1] + 1]) == -1                   # an N the blob was not prepared for
    assert b"prepared for N" in lib.tvc_last_error(eng.ctx)
    wav = torch.zeros(B, 4800, device=DEV)
    wave = torch.full((B, 4800), 7.0, device=DEV)
    arr = (ctypes.c_void_p * B)(ptrs[0], None)
    nn = (ctypes.c_int64 * B)(*ns)
    assert lib.tvc_convert_multi_f32(eng.ctx, eng._stream(), ctypes.c_void_p(wav.data_ptr()), arr, nn, 0.0, None, None, 1,
                                     ctypes.c_void_p(wave.data_ptr()), B, 4800, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel())) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((wave == 7.0).all()), "a refused call wrote its output"
    with pytest.raises(ValueError):
        eng.knn_match_multi(src, blobs[:1], ns[:1])              # a table of the wrong length
    with pytest.raises(ValueError):
        gen.convert(wav, targets[:3], 0.0)                       # three indices for two rows
    with pytest.raises(ValueError):
        gen.convert(wav, targets[:2], [1.0, 2.0, 3.0])           # three shifts for two rows
