"""Keep a share of the source's own content features in the fused conversion: a per-row alpha (tvc_knn_match_alpha_f32,
tvc_convert_alpha_f32, tvc_convert_ragged_alpha_f32; Generator.convert(alpha=), BatchedStreamInfer(alpha=)).

Contract: with mu what the alpha-less call writes for an element, src the same element of the tensor that was searched and a = alpha[row],
an alpha call writes mu * (1 - a) + src * a - the subtraction, the two products and the sum rounded separately: the bits of torch's eager
expression on fp32 tensors; the indices do not depend on alpha; a row with alpha 0 is the alpha-less row, a row with alpha 1 the source's; every
row of a batch (equal or ragged, at any input amplitude) equals its own B = 1 call; and a captured stream graph follows in-place changes of
alpha without a new capture."""
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
    """test_gpu_blend.py's four: the exact kernel (N = 300), the two-stage search (6 000), fp16 storage (12 000), another 6 000."""
    return [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV),
            synth.synth_index(12000, seed=23).half().to(DEV), synth.synth_index(6000, seed=24).to(DEV)]


@pytest.fixture(scope="module")
def src():
    """B = 3, T = 45: 135 query columns - the 32-column tiles straddle the row edges at 45 and 90, the last tile holds 7 columns"""
    return torch.randn(3, 768, 45, generator=torch.Generator().manual_seed(5))


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


# two alpha vectors: 0, one inside (0, 1), one outside [0, 1]; then 1, a negative one, 0 in another row
ALPHAS = [[0.0, 0.35, 1.5], [1.0, -0.25, 0.0]]


@pytest.mark.parametrize("form", ["table", "fp16", "blend"])
def test_stage_bits(targets, src, form):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    src_d = src.to(DEV)
    B = src.shape[0]
    w = None
    if form == "table":          # one index per row, N = 300 / 6 000 / 6 000: the exact kernel and the two-stage search in one call
        blobs, ns = prepare_references([targets[0], targets[1], targets[3]])
        mu, midx = eng.knn_match_multi(src_d, blobs, ns, want_indices=True)
        midx = midx[None]
    elif form == "fp16":         # one fp16-kind blob in every row
        blobs, ns = prepare_references([targets[2]] * B)
        mu, midx = eng.knn_match_multi(src_d, blobs, ns, want_indices=True)
        midx = midx[None]
    else:                        # M = 2, negative weights too
        w = torch.tensor([[0.7, 0.3], [1.2, -0.2], [0.5, 0.5]], device=DEV)
        blobs, ns = prepare_references([targets[(b + m) % 4] for b in range(B) for m in range(2)])
        mu, midx = eng.knn_match_blend(src_d, blobs, ns, w, want_indices=True)
    for alphas in ALPHAS:
        a = torch.tensor(alphas, device=DEV)
        out, idx = eng.knn_match_alpha(src_d, blobs, ns, a, weights=w, want_indices=True)
        a_t = a.view(B, 1, 1)
        assert torch.equal(out, mu * (1 - a_t) + src_d * a_t), f"{form} {alphas}: not the bits of torch's mu * (1 - a) + src * a"
        assert idx.shape == midx.shape and torch.equal(idx, midx), f"{form} {alphas}: the indices depend on alpha"
        for b, x in enumerate(alphas):
            if x == 0.0:
                assert torch.equal(out[b], mu[b]), f"{form}: the row with alpha 0 is not the alpha-less row"
            if x == 1.0:
                assert torch.equal(out[b], src_d[b]), f"{form}: the row with alpha 1 is not the source's"


def test_stage_against_the_oracle(targets, src):
    """oracle.ref_cpu.match_features(..., alpha=) on one index, row by row (it takes one alpha): test_gpu_parity.py's criterion for the general
    route - within 2e-7 of the output's |max|, indices equal.  synth_index(6000, seed=22) against this source keeps every top-5 gap above
    1e-5 (2.7e-5 at the least, found on the CPU with the oracle alone), so fp32 decides every index."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    B = src.shape[0]
    ref = targets[1]
    blobs, ns = prepare_references([ref] * B)
    alphas = ALPHAS[0]
    out, idx = eng.knn_match_alpha(src.to(DEV), blobs, ns, torch.tensor(alphas, device=DEV), want_indices=True)
    for b, a in enumerate(alphas):
        want, o_idx, sims = R.match_features(src[b:b + 1], ref.cpu(), return_indices=True, alpha=a)
        top = torch.topk(sims.double(), 5, dim=2).values
        assert float((top[..., :-1] - top[..., 1:]).min()) > 1e-5, "the oracle alone cannot decide this index"
        assert torch.equal(idx[0, b].cpu(), o_idx[0]), f"row {b}: indices differ from the oracle's"
        err = float((out[b:b + 1].cpu() - want).abs().max() / want.abs().max())
        print(f"[alpha] row {b} alpha {a}: {err:.2e} of the output's |max| vs the oracle")
        assert err <= 2e-7, (b, a, err)


def _oracle_alpha_convert(enc_sd, dec_sd, wf, ref, alpha, shift, angle):
    """the reference's convert (generator.py:26-34) with match_features given alpha"""
    with torch.inference_mode():
        wf = R.autopad_waveform(wf)
        spec = R.spectrogram(wf)
        energy = R.estimate_energy(wf)
        z, f0 = R.encoder_infer(enc_sd, spec)
        zm = R.match_features(z, ref, alpha=alpha)
        return R.decoder_infer(dec_sd, zm, R.shift_frequency(f0, shift), energy, angle)


B2, T2 = 2, 100
SHIFTS2, ALPHAS2 = [2.0, -3.0], [0.3, 1.1]


def _equal_case(scale=1.0):
    wf = synth.synth_wave(B2, T2 * 480, seed=41) * scale
    return wf, synth.synth_angle(B2, T2, 42).to(DEV)


def test_convert_equal_lengths(gen, targets):
    enc_sd, dec_sd = state_dicts(0)
    wf, angle = _equal_case()
    tg = [targets[1], targets[2]]
    out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b])
        assert torch.equal(out[b:b + 1], one), f"row {b}: the batched alpha call != its B = 1 call"
        with oracle_one_thread():
            ref = _oracle_alpha_convert(enc_sd, dec_sd, wf[b:b + 1], tg[b].float().cpu(), ALPHAS2[b], SHIFTS2[b], angle[b:b + 1].cpu())
        d = rms(out[b].cpu() - ref[0])
        print(f"[alpha] row {b}: {d:.3e} rms vs the oracle composition")
        assert d <= 1e-4, f"row {b}: {d:.3e} rms vs the oracle composition"
    plain = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle)
    assert not torch.equal(out, plain)
    # alpha all zero: the alpha-less call bit for bit (the bound is the index's exactly), as floats and as a device tensor used in place
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=0.0), plain)
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=torch.zeros(B2, device=DEV)), plain)
    # one shared index and one shift take the same entry
    shared = gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, alpha=[0.0, 0.0])
    assert torch.equal(shared, gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle))
    # a blend target
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    blend = Blend([[targets[0], targets[1]], [targets[2], targets[3]]], torch.tensor([[0.7, 0.3], [0.25, 0.75]], device=DEV))
    ob = gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, alpha=ALPHAS2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), Blend([blend.terms[0][b], blend.terms[1][b]], blend.weights[b].tolist()), SHIFTS2[b],
                          noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b])
        assert torch.equal(ob[b:b + 1], one), f"row {b}: the batched alpha blend != its B = 1 call"
    assert torch.equal(gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, alpha=0.0), gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle))


def test_convert_auto_pitch_shifts_do_not_depend_on_alpha(gen, targets):
    wf, angle = _equal_case()
    tg = [targets[1], targets[2]]
    reg = torch.tensor([180.0, 240.0], device=DEV)
    plain, sh0 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True)
    out, sh = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, alpha=ALPHAS2)
    assert torch.equal(sh, sh0), "the shifts found on the device depend on alpha"
    assert not torch.equal(out, plain) and torch.isfinite(out).all()
    zero, shz = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, alpha=0.0)
    assert torch.equal(zero, plain) and torch.equal(shz, sh0)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), auto_pitch=reg[b:b + 1].contiguous(),
                          alpha=ALPHAS2[b])
        assert torch.equal(out[b:b + 1], one), f"row {b}: the batched auto-pitch alpha call != its B = 1 call"


def test_convert_ragged(gen, targets):
    """test_gpu_blend.py::test_convert_ragged's frames - one row per length class, then eight rows under a frame cap that cuts the two upper
    classes into two in-kernel batches each - with an alpha of its own in every row: each row equals its own B = 1 alpha conversion over its
    own length (its content bound takes the |max| of ITS ssl)."""
    frames = [7, 150, 33, 60, 9, 131, 20, 90]
    lens = [480 * f - (11 if i % 2 else 0) for i, f in enumerate(frames)]
    alphas = [0.3, 1.25, 0.0, -0.4, 1.0, 0.5, 0.8, 0.05]
    B, Lmax, Tmax = len(frames), 480 * max(frames), max(frames)
    wf = torch.zeros(B, Lmax)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=600 + b)[0]
    tg = [targets[b % 4] for b in range(B)]
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    ones = [gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tg[b], -2.0, noise_angle=angle[b:b + 1, :, :f].contiguous(), alpha=alphas[b])
            for b, f in enumerate(frames)]
    eng = gen.engine()
    try:
        for rows, cap in ((4, 0), (4, 100), (8, 100)):
            eng.set_ragged_batch_frames(cap)
            a = torch.tensor(alphas[:rows], device=DEV)
            out = gen.convert(wf[:rows].to(DEV), tg[:rows], -2.0, noise_angle=angle[:rows].contiguous(), lengths=lens[:rows], alpha=a)
            for b in range(rows):
                f = frames[b]
                assert torch.equal(out[b, :480 * f], ones[b][0]), f"{rows} rows, cap {cap}: row {b} ({f} frames, alpha {alphas[b]})"
                assert not out[b, 480 * f:].any()
    finally:
        eng.set_ragged_batch_frames(0)


@pytest.mark.parametrize("scale", [1e4, 1e-7])
def test_range_guard(gen, targets, scale):
    """the equal-length case at two input amplitudes (test_gpu_ragged.py's): the content bound follows the source's own |max|"""
    wf, angle = _equal_case(scale)
    tg = [targets[1], targets[2]]
    out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2)
    assert torch.isfinite(out).all()
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b])
        assert torch.equal(out[b:b + 1], one), f"scale {scale}: row {b} != its B = 1 call"


def test_streams_follow_live_alpha_without_a_new_capture(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk = 2, 8
    tg = [targets[0], synth.synth_index(800, seed=83).to(DEV)]
    a0, new = [0.2, 0.9], torch.tensor([0.75, -0.1])
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)
    sts = {}
    for use_graph in (True, False):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840,
                                use_graph=use_graph, alpha=a0)
        st.init_buffer()
        assert st.alpha.shape == (S,) and st.alpha.dtype == torch.float32 and st.alpha.device == torch.device(DEV)
        sts[use_graph] = st

    def block(i):
        angle = synth.synth_angle(S, sts[True].input_size // 480, 850 + i).to(DEV)
        return [sts[g].audio_callback(blocks[:, i], noise_angle=angle).clone() for g in (True, False)]

    outs = []
    for i in range(4):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        outs.append(a)
    graph3 = sts[True]._graph[1][True][0]                        # captured at block 3
    for g in (True, False):
        sts[g].alpha.copy_(new)                                  # the knob moves: in place, on the device
    for i in range(4, nblk):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: the replay did not follow the new alpha"
        assert sts[True]._graph[1][True][0] is graph3, "changing alpha in place must not capture again"
    # and the knob does something: the same blocks without alpha differ
    st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840)
    st.init_buffer()
    assert st.alpha is None
    y = st.audio_callback(blocks[:, 0], noise_angle=synth.synth_angle(S, st.input_size // 480, 850).to(DEV))
    assert not torch.equal(y, outs[0])


def test_stream_with_tracker_and_door_in_one_graph(gen, targets):
    """alpha beside a live pitch tracker and a door at 48 kHz: one captured block, equal to the eager stream block for block"""
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor
    S, nblk = 2, 6
    tg = [targets[0], targets[1]]
    sts = {}
    for use_graph in (True, False):
        door = StreamDoor(S, 48000, block_size=1920, device=DEV)
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=0.5, device=torch.device(DEV), block_size=1920, extra_size=3840, use_graph=use_graph,
                                door=door, auto_pitch=torch.tensor([200.0, 150.0], device=DEV), alpha=[0.4, 0.0])
        st.init_buffer()
        sts[use_graph] = st
    chunk = sts[True].door.chunk_in
    pcm = (synth.synth_wave(S, nblk * chunk, seed=91) * 20000).clamp(-32768, 32767).to(torch.int16).view(S, nblk, chunk).to(DEV)
    for i in range(nblk):
        if i == 4:
            for g in (True, False):
                sts[g].alpha.fill_(0.6)
        angle = synth.synth_angle(S, sts[True].input_size // 480, 950 + i).to(DEV)
        a, b = [sts[g].audio_callback_pcm(pcm[:, i], noise_angle=angle).clone() for g in (True, False)]
        assert a.dtype == torch.int16 and torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(sts[True].last_pitch_shift, sts[False].last_pitch_shift)
    assert len(sts[True]._graph[1]) == 1, "one captured block"


def test_refusals(gen, targets, src):
    """an alpha the entries cannot take is refused on the host, under its name, before anything is launched"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    B = src.shape[0]
    src_d = src.to(DEV)
    blobs, ns = prepare_references([targets[0]] * B)
    for bad, exc in ((torch.zeros(B + 1, device=DEV), ValueError), (torch.zeros(B, dtype=torch.float64, device=DEV), ValueError),
                     (torch.zeros(B, 1, device=DEV), ValueError), (torch.zeros(B), RuntimeError), ([0.0] * B, TypeError), (0.5, TypeError)):
        with pytest.raises(exc, match="alpha"):
            eng.knn_match_alpha(src_d, blobs, ns, bad)
    wf = synth.synth_wave(2, 9600, seed=1).to(DEV)
    angle = synth.synth_angle(2, 20, 3).to(DEV)
    before = torch.cuda.get_rng_state(DEV).clone()
    for bad in (torch.zeros(2), torch.zeros(3, device=DEV), torch.zeros(2, dtype=torch.float16, device=DEV), [0.1, 0.2, 0.3], "0.5", True):
        with pytest.raises(ValueError, match="alpha"):
            gen.convert(wf, targets[0], 0.0, noise_angle=angle, alpha=bad)
        with pytest.raises(ValueError, match="alpha"):
            gen.convert(wf, targets[0], 0.0, alpha=bad)      # refused before the noise draw
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)
