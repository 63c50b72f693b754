"""Convert toward a weighted blend of speaker indices in one call (tvc_knn_match_blend_f32, tvc_convert_blend_f32,
tvc_convert_ragged_blend_f32; feature_retrieval.Blend).

Contract: with mu_m = the single-index match of a row against term m's blob, a blend call writes w_0 * mu_0, then + w_m * mu_m in term
order, products and sums rounded separately - bit for bit the torch composition of the per-term calls; every term's indices are its own
call's; M = 1 / w = 1 is the multi-index call and weights (1, 0) the first term alone; every row of a batch (equal or ragged) equals its
own B = 1 blend call; and a captured stream graph follows in-place weight changes without a new capture."""
import pytest
import torch

from helpers import oracle_one_thread, rms, state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import audio_io, synth

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
    """test_gpu_multi_index.py's four: the exact kernel (N = 300), the two-stage search (6 000), fp16 storage (12 000), another 6 000."""
    return [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV),
            synth.synth_index(12000, seed=23).half().to(DEV), synth.synth_index(6000, seed=24).to(DEV)]


@pytest.fixture(scope="module")
def src():
    return torch.randn(3, 768, 333, generator=torch.Generator().manual_seed(5))      # B = 3, T = 333: partial query tiles in every segment


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _compose(eng, src_d, blend, w):
    """the staged route on the device: one knn_match per (row, term), then separate mul and add ops in term order -> (out, idx [M, B, T, 4])"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_reference
    B, M = src_d.shape[0], blend.M
    rows, idx = [], [[None] * B for _ in range(M)]
    for b in range(B):
        acc = None
        for m in range(M):
            t = blend.terms[m]
            t = t[b] if isinstance(t, (list, tuple)) else (t if t.shape[0] == 1 else t[b:b + 1].clone())
            blob, n = prepare_reference(t)
            mu, idx[m][b] = eng.knn_match(src_d[b:b + 1], blob, n, want_indices=True)
            term = torch.mul(w[b, m], mu)
            acc = term if m == 0 else torch.add(acc, term)
        rows.append(acc)
    return torch.cat(rows, 0), torch.stack([torch.cat(r, 0) for r in idx], 0)


def test_stage_bits_and_the_oracle(targets, src):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, match_features_blend
    eng = _engine()
    B, M = 3, 3
    w = (torch.rand(B, M, generator=torch.Generator().manual_seed(6)) * 2.0 - 0.5).to(DEV)      # in [-0.5, 1.5]: negative weights too
    blend = Blend([[targets[(b + m) % 4] for b in range(B)] for m in range(M)], w)
    assert blend.weights is w                                       # a [B, M] fp32 device tensor is used in place
    src_d = src.to(DEV)
    out, idx = match_features_blend(src_d, blend, return_indices=True)
    ref, ridx = _compose(eng, src_d, blend, w)
    assert idx.shape == (M, B, 333, 4)
    assert torch.equal(idx, ridx), "a term's indices differ from its own single-index call"
    assert torch.equal(out, ref), "the blend differs from the torch composition of the per-term calls"
    # the oracle, per term, wherever fp32 can decide the top 4 (fp16 term: on the same fp16-rounded vectors)
    for m in range(M):
        for b in range(B):
            _o, r_idx, sims = R.match_features(src[b:b + 1], targets[(b + m) % 4].float().cpu(), return_indices=True)
            top = torch.topk(sims, 5, dim=2).values
            ok = (top[..., :-1] - top[..., 1:]).min(dim=2).values > 1e-5
            assert ok.float().mean() > 0.9
            assert torch.equal(idx[m, b].cpu()[ok[0]], r_idx[0][ok[0]]), f"term {m}, row {b}: indices differ from the oracle on decidable columns"


def test_degenerate_forms(targets, src):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, match_features_blend, prepare_reference, prepare_references
    eng = _engine()
    src_d = src.to(DEV)
    B = src.shape[0]
    # M = 1, w = 1: the multi-index call
    tg = [targets[b % 4] for b in range(B)]
    blobs, ns = prepare_references(tg)
    multi, midx = eng.knn_match_multi(src_d, blobs, ns, want_indices=True)
    out, idx = match_features_blend(src_d, Blend([tg], [1.0]), return_indices=True)
    assert torch.equal(out, multi) and torch.equal(idx[0], midx)
    # M = 2, w = (1, 0): the first term alone (the second is searched, and contributes +0)
    blob, n = prepare_reference(targets[1])
    first, fidx = eng.knn_match(src_d, blob, n, want_indices=True)
    out, idx = match_features_blend(src_d, Blend([targets[1], targets[2]], [1.0, 0.0]), return_indices=True)
    assert torch.equal(out, first) and torch.equal(idx[0], fidx)
    # M = 4, one blob in every term: every term finds what the single call finds
    out, idx = match_features_blend(src_d, Blend([targets[1]] * 4, (0.25,) * 4), return_indices=True)
    for m in range(4):
        assert torch.equal(idx[m], fidx), f"term {m}"
    assert torch.isfinite(out).all()


def test_overflow_stays_per_term_and_row():
    """test_knn_multi_overflow_falls_back_per_segment's dense neighbourhood as term 1 of row 1 only: that (term, row) segment alone takes the
    exact kernel, every term still finds what its own call finds and the output is the composition."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, match_features_blend
    eng = _engine()
    T, B, M = 100, 2, 2
    g = torch.Generator().manual_seed(9)
    s = torch.randn(B, 768, T, generator=g)
    dense = torch.randn(1, 768, 5000, generator=g)
    dense[0, :, :400] = s[1, :, :1] + 1e-4 * torch.randn(768, 400, generator=g)      # 400 near-copies of row 1's first query
    w = torch.tensor([[0.6, 0.4], [0.3, 0.7]], device=DEV)
    blend = Blend([[synth.synth_index(5000, seed=31).to(DEV), synth.synth_index(5000, seed=32).to(DEV)],
                   [synth.synth_index(5000, seed=33).to(DEV), dense.to(DEV)]], w)
    out, idx = match_features_blend(s.to(DEV), blend, return_indices=True)
    ref, ridx = _compose(eng, s.to(DEV), blend, w)
    assert torch.equal(idx, ridx) and torch.equal(out, ref)
    assert int(idx[1, 1, 0].max()) < 400


def _oracle_blend_convert(enc_sd, dec_sd, wf, refs, w, shift, angle):
    """the reference's convert (generator.py:26-34) with the match replaced by the weighted sum of one match per term, in fp32"""
    with torch.inference_mode():
        wf = R.autopad_waveform(wf)
        spec = R.spectrogram(wf)
        energy = R.estimate_energy(wf)
        z, f0 = R.encoder_infer(enc_sd, spec)
        zm = None
        for m, ref in enumerate(refs):
            term = w[m] * R.match_features(z, ref)
            zm = term if m == 0 else zm + term
        return R.decoder_infer(dec_sd, zm, R.shift_frequency(f0, shift), energy, angle)


def test_convert_equal_lengths(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    enc_sd, dec_sd = state_dicts(0)
    B, T = 2, 100
    wf = synth.synth_wave(B, T * 480, seed=41)
    angle = synth.synth_angle(B, T, 42).to(DEV)
    shifts = [2.0, -3.0]
    terms = [[targets[0], targets[1]], [targets[2], targets[3]]]
    w = [[0.7, 0.3], [0.25, 0.75]]
    out = gen.convert(wf.to(DEV), Blend(terms, torch.tensor(w, device=DEV)), shifts, noise_angle=angle)
    worst = 0.0
    for b in range(B):
        one = gen.convert(wf[b:b + 1].to(DEV), Blend([terms[0][b], terms[1][b]], w[b]), shifts[b], noise_angle=angle[b:b + 1].contiguous())
        assert torch.equal(out[b:b + 1], one), f"row {b}: the batched blend != its B = 1 blend call"
        with oracle_one_thread():
            ref = _oracle_blend_convert(enc_sd, dec_sd, wf[b:b + 1], [terms[0][b].float().cpu(), terms[1][b].float().cpu()], w[b], shifts[b],
                                        angle[b:b + 1].cpu())
        d = rms(out[b].cpu() - ref[0])
        worst = max(worst, d)
        print(f"[blend] row {b}: {d:.3e} rms vs the oracle composition")
        assert d <= 1e-4, f"row {b}: {d:.3e} rms vs the oracle composition"
    print(f"[blend] worst rms vs the oracle composition {worst:.3e}")
    # weights (1, 0): the bound and the content are the first terms' alone - today's multi-index call bit for bit
    first = gen.convert(wf.to(DEV), Blend(terms, [[1.0, 0.0], [1.0, 0.0]]), shifts, noise_angle=angle)
    assert torch.equal(first, gen.convert(wf.to(DEV), terms[0], shifts, noise_angle=angle))


def test_convert_ragged(gen, targets):
    """One row per length class (the four rows the kernels choose differently for), then eight rows under a frame cap that cuts the two
    upper classes into two in-kernel batches each: every row equals its own B = 1 blend conversion over its own length."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    frames = [7, 150, 33, 60, 9, 131, 20, 90]
    lens = [480 * f - (11 if i % 2 else 0) for i, f in enumerate(frames)]
    B, Lmax, Tmax = len(frames), 480 * max(frames), max(frames)
    wf = torch.zeros(B, Lmax)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=600 + b)[0]
    terms = [[targets[b % 4] for b in range(B)], [targets[(b + 1) % 4] for b in range(B)]]
    w = torch.rand(B, 2, generator=torch.Generator().manual_seed(62)) * 1.5 - 0.25
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    ones = [gen.convert(wf[b:b + 1, :lens[b]].to(DEV), Blend([terms[0][b], terms[1][b]], w[b].tolist()), -2.0,
                        noise_angle=angle[b:b + 1, :, :f].contiguous()) for b, f in enumerate(frames)]
    eng = gen.engine()
    try:
        for rows, cap in ((4, 0), (4, 100), (8, 100)):
            eng.set_ragged_batch_frames(cap)
            blend = Blend([terms[0][:rows], terms[1][:rows]], w[:rows].to(DEV))
            out = gen.convert(wf[:rows].to(DEV), blend, -2.0, noise_angle=angle[:rows].contiguous(), lengths=lens[:rows])
            for b in range(rows):
                f = frames[b]
                assert torch.equal(out[b, :480 * f], ones[b][0]), f"{rows} rows, cap {cap}: row {b} ({f} frames)"
                assert not out[b, 480 * f:].any()
    finally:
        eng.set_ragged_batch_frames(0)


def test_streams_follow_live_weights_without_a_new_capture(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    S, nblk = 2, 8
    shared = synth.synth_index(300, seed=81).to(DEV)
    own = [synth.synth_index(5000, seed=82).to(DEV), synth.synth_index(800, seed=83).to(DEV)]
    w0 = torch.tensor([[0.7, 0.3], [0.2, 0.8]])
    new = torch.tensor([[0.1, 0.9], [1.3, -0.3]])
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)
    sts, blends = {}, {}
    for use_graph in (True, False):
        blends[use_graph] = Blend([shared, list(own)], w0.to(DEV))
        st = BatchedStreamInfer(gen, n_streams=S, target=blends[use_graph], pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920,
                                extra_size=3840, use_graph=use_graph)
        st.init_buffer()
        sts[use_graph] = st

    def block(i):
        angle = synth.synth_angle(S, sts[True].input_size // 480, 850 + i).to(DEV)
        return [sts[g].audio_callback(blocks[:, i], noise_angle=angle).clone() for g in (True, False)]

    for i in range(4):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
    graph3 = sts[True]._graph[1][True][0]                        # captured at block 3
    for g in (True, False):
        blends[g].weights.copy_(new)                             # the slider moves: in place, on the device
    for i in (4, 5):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: the replay did not follow the new weights"
        assert sts[True]._graph[1][True][0] is graph3, "changing the weights in place must not capture again"
    other = synth.synth_index(700, seed=85).to(DEV)
    for g in (True, False):
        blends[g].terms[0] = other                               # another index: the tables are kernel arguments, so this captures again
    for i in (6, 7):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager behind a swapped term"
    assert sts[True]._graph[1][True][0] is not graph3


def test_infer_py_blend_with_a_zero_weight_is_the_single_index_run(tmp_path):
    import infer
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(300, seed=2), d / "a.pt")
    torch.save(synth.synth_index(500, seed=4), d / "b.pt")
    (d / "inputs").mkdir()
    audio_io.save(str(d / "inputs" / "x.wav"), synth.synth_wave(1, 12000, seed=3) * 0.9, 24000)
    common = ["-i", str(d / "inputs"), "-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-p", "1.0", "-d", "cuda:0", "--seed", "3"]
    assert infer.main(common + ["-o", str(d / "out_blend"), "--blend", f"{d / 'a.pt'}=1", f"{d / 'b.pt'}=0"]) == 0
    assert infer.main(common + ["-o", str(d / "out_idx"), "-idx", str(d / "a.pt")]) == 0
    got, want = open(d / "out_blend" / "x.wav", "rb").read(), open(d / "out_idx" / "x.wav", "rb").read()
    assert len(want) > 12000 * 2 and got == want
