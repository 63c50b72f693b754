"""Building a speaker index in one pass on the device: ragged encode (tvc_encode_ragged_f32), the gather into a prepared blob
(tvc_knn_prepare_index_cols_f32 / _f16), build_index and extract_index.py --batch-frames.

The reference encodes the clips of a speaker one by one, subsamples, concatenates, permutes and truncates on the host
(extract_index.py:43-58).  The contracts here are exact: every clip of a ragged encode equals its own `encode`, the gathered blob
equals the blob prepared from the selected tensor byte for byte, and the batched script writes the file the clip-by-clip run writes."""
import ctypes

import pytest
import torch

from helpers import oracle_one_thread, state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FRAMES = [3, 10, 11, 42, 43, 64, 65, 130]      # the shortest legal input, both sides of the 11 / 43 / 128 length classes and of the 64-column GRN / LayerNorm tile
LENS = [480 * f - (17 if i % 2 else 0) for i, f in enumerate(FRAMES)]      # odd rows are not yet padded to a frame


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
def clips():
    wf = torch.zeros(len(FRAMES), 480 * max(FRAMES))
    for b, n in enumerate(LENS):
        wf[b, :n] = synth.synth_wave(1, n, seed=500 + b)[0]
    return wf


@pytest.fixture(scope="module")
def ragged(gen, clips):
    """One ragged encode of the eight clips: (packed ssl [768, S], packed f0 [S], pre)."""
    ssl, f0, pre = gen.encode_packed(clips.to(DEV), LENS)
    return ssl.clone(), f0.clone(), pre


def test_ragged_encode_equals_one_call_per_utterance_and_the_oracle(gen, clips, ragged):
    enc_sd, _ = state_dicts(0)
    ssl, f0p, pre = ragged
    assert pre == [sum(FRAMES[:b]) for b in range(len(FRAMES) + 1)] and ssl.shape == (768, sum(FRAMES)) and f0p.shape == (sum(FRAMES),)
    tgt, f0 = gen.encode(clips.to(DEV), lengths=LENS)
    assert len(tgt) == len(f0) == len(FRAMES)
    worst = 0.0
    for b, t in enumerate(FRAMES):
        assert tgt[b].shape == (1, 768, t) and f0[b].shape == (1, 1, t)
        assert tgt[b].data_ptr() == tgt[0].data_ptr() + 4 * pre[b], "the features are views of ONE packed tensor"
        assert torch.equal(tgt[b][0], ssl[:, pre[b]:pre[b + 1]]) and torch.equal(f0[b][0, 0], f0p[pre[b]:pre[b + 1]])
        one, one_f0 = gen.encode(clips[b:b + 1, :LENS[b]].to(DEV))
        assert torch.equal(tgt[b], one), f"utterance {b} ({t} frames): ragged encode != its own encode"
        assert torch.equal(f0[b], one_f0), f"utterance {b} ({t} frames): f0 of the ragged encode != its own encode"
        with oracle_one_thread():
            want, _ = R.encode(enc_sd, clips[b:b + 1, :LENS[b]])
        got = tgt[b].cpu().double()
        err = (got - want.double()).pow(2).sum(dim=1).sqrt() / want.double().pow(2).sum(dim=1).sqrt()      # per column
        worst = max(worst, float(err.max()))
    print(f"[index build] ragged encode of {FRAMES} frames: every utterance equals its own encode bit for bit; worst column rel error vs the oracle {worst:.2e}")
    assert worst < 1e-5


def test_several_in_kernel_batches_write_the_same_packed_outputs(gen, clips, ragged):
    ssl, f0p, pre = ragged
    eng = gen.engine(DEV)
    eng.set_ragged_batch_frames(100)             # [3 10 11 42] [43] [64] [65] [130]: five batches, the later ones placed by the pack kernel
    try:
        ssl2, f02, pre2 = gen.encode_packed(clips.to(DEV), LENS)
    finally:
        eng.set_ragged_batch_frames(0)
    assert pre2 == pre
    assert torch.equal(ssl2, ssl) and torch.equal(f02, f0p), "the packed outputs depend on the cut into batches (or left the caller's row order)"


def test_ragged_encode_arguments_are_validated(gen):
    from tinyvc_amd._lib import TinyVCError
    wf = torch.zeros(2, 4800, device=DEV)
    with pytest.raises(ValueError):
        gen.encode(wf, lengths=[4800, 900])              # torch.stft's reflect padding needs more than 960 samples
    with pytest.raises(ValueError):
        gen.encode(wf, lengths=[4800, 9600])             # longer than its row
    with pytest.raises(ValueError):
        gen.encode(wf, lengths=[4800])                   # one entry per row
    with pytest.raises(TinyVCError):
        gen.engine(DEV).encode_ragged(wf, [4800, 960])   # the C call refuses what tvc_convert_ragged_f32 refuses


# ---- gather into a prepared blob ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gather_inputs():
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(768, 700, generator=g)
    scale = torch.ones(700)
    scale[::7] = 1e-3 / 768 ** 0.5                       # columns with norm near 1e-3 ...
    scale[3::7] = 1e3 / 768 ** 0.5                       # ... and near 1e3
    feats = (feats * scale).contiguous()
    cols = torch.randperm(700, generator=g)[:300].clone()
    cols[1], cols[2], cols[126], cols[200] = 0, 699, int(cols[0]), int(cols[5])      # both ends of the tensor, two duplicated columns
    queries = torch.randn(1, 768, 50, generator=g)
    return feats.to(DEV), cols.to(DEV), queries.to(DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("N", [4, 127, 128, 129, 300])      # the smallest legal index, both sides of a 128-vector image tile, several tiles
def test_gather_prepare_equals_select_then_prepare_byte_for_byte(gather_inputs, N):
    from tinyvc_amd.engine import default_engine
    feats, cols, queries = gather_inputs
    cols = cols[:N].contiguous()
    eng = default_engine(torch.device(DEV))
    lib, st = eng.lib, eng._stream()
    sel = feats[:, cols].contiguous()
    # fp32 storage
    want = torch.zeros(lib.tvc_knn_prepared_elems(N), device=DEV)
    got = torch.zeros_like(want)
    out = torch.full((768, N), float("nan"), device=DEV)
    eng._ok(lib.tvc_knn_prepare_index_f32(eng.ctx, st, _ptr(sel), _ptr(want), N), "tvc_knn_prepare_index_f32")
    eng._ok(lib.tvc_knn_prepare_index_cols_f32(eng.ctx, st, _ptr(feats), 700, _ptr(cols), N, _ptr(got), _ptr(out)), "tvc_knn_prepare_index_cols_f32")
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
    assert diff.numel() == 0, f"fp32 blob differs in {diff.numel()} words, first at {diff[:8].tolist()} of {want.numel()}"
    assert torch.equal(out, sel)
    a, ia = eng.knn_match(queries, want, N, want_indices=True)
    b, ib = eng.knn_match(queries, got, N, want_indices=True)
    assert torch.equal(ia, ib) and torch.equal(a, b)
    got.zero_()                                               # index_out = NULL: the blob alone
    eng._ok(lib.tvc_knn_prepare_index_cols_f32(eng.ctx, st, _ptr(feats), 700, _ptr(cols), N, _ptr(got), None), "tvc_knn_prepare_index_cols_f32")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # fp16 storage
    rows16 = sel.t().half().contiguous()
    want16 = torch.zeros(lib.tvc_knn_prepared_elems_f16(N), device=DEV)
    got16 = torch.zeros_like(want16)
    out16 = torch.full((768, N), float("nan"), dtype=torch.float16, device=DEV)
    eng._ok(lib.tvc_knn_prepare_index_f16(eng.ctx, st, _ptr(rows16), _ptr(want16), N), "tvc_knn_prepare_index_f16")
    eng._ok(lib.tvc_knn_prepare_index_cols_f16(eng.ctx, st, _ptr(feats), 700, _ptr(cols), N, _ptr(got16), _ptr(out16)), "tvc_knn_prepare_index_cols_f16")
    diff = (got16.view(torch.int32) != want16.view(torch.int32)).nonzero().flatten()
    assert diff.numel() == 0, f"fp16 blob differs in {diff.numel()} words, first at {diff[:8].tolist()} of {want16.numel()}"
    assert torch.equal(out16, sel.half())
    a, ia = eng.knn_match(queries, want16, N, want_indices=True)
    b, ib = eng.knn_match(queries, got16, N, want_indices=True)
    assert torch.equal(ia, ib) and torch.equal(a, b)
    for blob in (want, got, want16, got16):                   # (the library remembers blobs by address: these go back to the allocator)
        lib.tvc_knn_forget(eng.ctx, _ptr(blob))


def test_gather_prepare_arguments_are_validated():
    from tinyvc_amd.engine import default_engine
    eng = default_engine(torch.device(DEV))
    lib = eng.lib
    x = torch.zeros(768, 8, device=DEV)
    c = torch.zeros(4, dtype=torch.int64, device=DEV)
    blob = torch.zeros(lib.tvc_knn_prepared_elems(4), device=DEV)
    for fn in (lib.tvc_knn_prepare_index_cols_f32, lib.tvc_knn_prepare_index_cols_f16):
        assert fn(eng.ctx, eng._stream(), None, 8, _ptr(c), 4, _ptr(blob), None) != 0
        assert fn(eng.ctx, eng._stream(), _ptr(x), 8, None, 4, _ptr(blob), None) != 0
        assert fn(eng.ctx, eng._stream(), _ptr(x), 0, _ptr(c), 4, _ptr(blob), None) != 0
        assert fn(eng.ctx, eng._stream(), _ptr(x), 8, _ptr(c), 0, _ptr(blob), None) != 0
        assert fn(None, eng._stream(), _ptr(x), 8, _ptr(c), 4, _ptr(blob), None) != 0
    with pytest.raises(ValueError):
        eng.knn_prepare_columns(torch.zeros(767, 8, device=DEV), c)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
CLIP_LENS = (24000, 31200 - 77, 19200 + 5)                   # 50, 65 and 41 frames once padded


def test_build_index_equals_the_index_assembled_from_one_encode_per_clip(gen):
    from tinyvc_amd.engine import Engine
    from tinyvc_amd.module.tinyvc import build_index
    wf = torch.zeros(3, 31200)
    for b, n in enumerate(CLIP_LENS):
        wf[b, :n] = synth.synth_wave(1, n, seed=40 + b)[0]
    wf = wf.to(DEV)
    supply = sum(-(-(-(-n // 480)) // 4) for n in CLIP_LENS)
    assert supply == 13 + 17 + 11
    perm = torch.randperm(supply, generator=torch.Generator().manual_seed(7))
    feats = torch.cat([gen.encode(wf[b:b + 1, :n])[0][:, :, ::4] for b, n in enumerate(CLIP_LENS)], dim=2)
    want = feats.index_select(2, perm.to(DEV))[:, :, :30].contiguous()
    calls = []
    orig = Engine.knn_prepare

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    src = synth.synth_wave(1, 9600, seed=3).to(DEV)
    angle = synth.synth_angle(1, 20, 5).to(DEV)
    Engine.knn_prepare = spy
    try:
        got = build_index(gen, wf, list(CLIP_LENS), stride=4, size=30, perm=perm)
        assert got.shape == (1, 768, 30) and got.dtype == torch.float32
        assert torch.equal(got, want)
        out = gen.convert(src, got, 1.0, noise_angle=angle)
        assert not calls, "build_index hands its prepared blob on: the first convert prepares nothing"
    finally:
        Engine.knn_prepare = orig
    ref = gen.convert(src, want, 1.0, noise_angle=angle)
    assert torch.equal(out, ref)
    half = build_index(gen, wf, list(CLIP_LENS), stride=4, size=30, perm=perm, half=True)
    assert half.dtype == torch.float16 and torch.equal(half, want.half())
    assert torch.equal(gen.convert(src, half, 1.0, noise_angle=angle), gen.convert(src, want.half(), 1.0, noise_angle=angle))


def test_extract_index_batch_frames_writes_the_same_file(tmp_path):
    import extract_index
    from tinyvc_amd.engine import Engine
    d = tmp_path / "clips"
    d.mkdir()
    torch.save(synth.synth_state_dict("encoder"), tmp_path / "encoder.pt")
    for i, n in enumerate(CLIP_LENS):
        audio_io.save(str(d / f"{i}.wav"), synth.synth_wave(1, n, seed=40 + i), 24000)
    common = ["--dataset-cache", str(d), "-encp", str(tmp_path / "encoder.pt"), "-size", "30", "-d", DEV, "--seed", "7"]
    calls = []
    orig = Engine.encode_ragged

    def spy(self, wav, lengths):
        calls.append(list(lengths))
        return orig(self, wav, lengths)

    for extra in ([], ["--half"]):
        assert extract_index.main(common + extra + ["-o", str(tmp_path / "loop.pt")]) == 0
        a = torch.load(tmp_path / "loop.pt")
        for cap in ("100", "120"):      # seed 7 takes the clips as 50, 65, 41 frames: three calls under a cap of 100, [50 65] [41] under 120
            del calls[:]
            Engine.encode_ragged = spy
            try:
                assert extract_index.main(common + extra + ["-o", str(tmp_path / "batched.pt"), "--batch-frames", cap]) == 0
            finally:
                Engine.encode_ragged = orig
            assert len(calls) >= 2 and all(sum(c) <= int(cap) * 480 for c in calls), calls
            assert sorted(sum(calls, [])) == sorted(-(-n // 480) * 480 for n in CLIP_LENS), calls
            assert cap == "100" or max(len(c) for c in calls) > 1, calls
            b = torch.load(tmp_path / "batched.pt")
            assert a.shape == b.shape == (1, 768, 30) and a.dtype == b.dtype == (torch.float16 if extra else torch.float32)
            assert torch.equal(a, b)
