"""protect: a per-frame share of the source from the call's own f0 (tvc_frame_share_f32, tvc_knn_match_protect_f32, tvc_convert_protect_f32,
tvc_convert_ragged_protect_f32; Generator.convert(protect=), BatchedStreamInfer(protect=)).

Contract (include/tinyvc_hip.h): with u[t] = f0[t] > 0 over ONE utterance, w[t] = 1 - (u[t-1] + 2 u[t] + u[t+1]) / 4 (edges repeated),
a = alpha[row] and p = protect[row], frame t keeps a_t = a + (1 - a) * (p * w[t]) of the source and every element of its column leaves as
mu * (1 - a_t) + src * a_t - the bits of torch's eager expressions on fp32 tensors (restated in tests/test_protect_host.py).  The indices do
not depend on p, p = 0 is the alpha call bit for bit, every row of a batch (equal or ragged, at any amplitude) equals its own B = 1 call, and
a captured stream graph follows in-place changes of protect without a new capture."""
import pytest
import torch

from helpers import F0_PATTERNS, dsp_edge_f0, oracle_one_thread, rms, state_dicts
from oracle import ref_cpu as R
from test_protect_host import frame_share, frame_weights
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
    """test_gpu_alpha.py's four: the exact kernel (N = 300), the two-stage search (6 000), fp16 storage (12 000), another 6 000."""
    return [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV),
            synth.synth_index(12000, seed=23).half().to(DEV), synth.synth_index(6000, seed=24).to(DEV)]


@pytest.fixture(scope="module")
def src():
    """test_gpu_alpha.py's: B = 3, T = 45 - the 32-column tiles straddle the row edges at 45 and 90, the last tile holds 7 columns"""
    return torch.randn(3, 768, 45, generator=torch.Generator().manual_seed(5))


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


# ---- 1. the frame-share kernel alone --------------------------------------------------------------------------------------------------
ROW_FRAMES = [3, 64, 1, 257, 28]
ALPHAS, PROTECTS = [0.0, 0.35, 1.5, -0.25], [0.0, 0.5, 1.0]


@pytest.mark.parametrize("pattern", F0_PATTERNS)
def test_frame_share_bits(pattern):
    """packed rows of 3, 64, 1, 257 and 28 frames in one launch (the 257-frame row spans two workgroups), NaN poison in front, between and
    behind; then a row whose last frame is unvoiced directly in front of a row whose first frame is voiced - neither may see the other -, and
    a row holding NaN and negative f0.  Every (alpha, protect) pair over the three launches."""
    eng = _engine()
    rows = [dsp_edge_f0(pattern, 1, T)[0, 0] for T in ROW_FRAMES]
    tail, head = 60.0 + torch.arange(6.0), 90.0 + torch.arange(5.0)
    tail[-1] = 0.0                                    # ... unvoiced last frame | voiced first frame, no gap between the two rows
    odd = torch.tensor([110.0, float("nan"), 120.0, -3.0, 130.0, 140.0, float("nan"), float("nan"), 150.0, -0.0, 160.0])
    rows += [tail, head, odd]
    gaps = [5, 2, 1, 3, 7, 4, 0, 2, 6]                # NaN columns in front of every row (none between `tail` and `head`) and behind the last
    packed, start = [], []
    for gap, row in zip(gaps, rows):
        packed.append(torch.full((gap,), float("nan")))
        start.append(sum(x.numel() for x in packed))
        packed.append(row)
    packed.append(torch.full((gaps[-1],), float("nan")))
    f0 = torch.cat(packed).to(DEV)
    counts = [r.numel() for r in rows]
    covered = torch.zeros(f0.numel(), dtype=torch.bool)
    for s, n in zip(start, counts):
        covered[s:s + n] = True
    for k in range(3):
        al = [ALPHAS[i % 4] for i in range(len(rows))]
        pr = [PROTECTS[(i + k) % 3] for i in range(len(rows))]
        got = eng.frame_share(f0, start, counts, torch.tensor(al, device=DEV), torch.tensor(pr, device=DEV)).cpu()
        for i, (s, n) in enumerate(zip(start, counts)):
            want = frame_share(rows[i], al[i], pr[i])
            assert torch.equal(got[s:s + n], want), f"{pattern}: row {i} ({n} frames, alpha {al[i]}, protect {pr[i]})"
        assert not got[~covered].any(), f"{pattern}: a column outside every row was written"
    # alpha None is alpha 0
    pr = torch.tensor([PROTECTS[i % 3] for i in range(len(rows))], device=DEV)
    assert torch.equal(eng.frame_share(f0, start, counts, None, pr), eng.frame_share(f0, start, counts, torch.zeros(len(rows), device=DEV), pr))


# ---- 2. the stage call ----------------------------------------------------------------------------------------------------------------
def _stage_f0():
    """[3, 45]: voicing changes at columns 31/32 (inside a tile), 44/45 (the row edge: unvoiced | voiced) and 89/90 (voiced | the
    all-unvoiced row), two short unvoiced runs and a NaN inside row 1"""
    f0 = 100.0 + torch.arange(135.0).view(3, 45)
    f0[0, 32:] = 0.0
    f0[1, 10:12] = 0.0
    f0[1, 20] = float("nan")
    f0[2] = 0.0
    return f0


# (alpha, protect) per row: row 0 of the first set has a = 0, p = 1 over voiced and unvoiced frames, row 2 of the second over unvoiced ones only
STAGE_SETS = [([0.0, 0.35, 1.5], [1.0, 0.5, 0.25]), ([1.0, -0.25, 0.0], [0.5, 1.0, 1.0])]


@pytest.mark.parametrize("form", ["table", "fp16", "blend"])
def test_stage_bits(targets, src, form):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    src_d = src.to(DEV)
    B, _, T = src.shape
    f0 = _stage_f0()
    f0_d = f0.to(DEV)
    w = None
    if form == "table":          # one index per row, N = 300 / 6 000 / 6 000: the exact kernel and the two-stage search in one call
        blobs, ns = prepare_references([targets[0], targets[1], targets[3]])
        mu, midx = eng.knn_match_multi(src_d, blobs, ns, want_indices=True)
        midx = midx[None]
    elif form == "fp16":         # one fp16-kind blob in every row
        blobs, ns = prepare_references([targets[2]] * B)
        mu, midx = eng.knn_match_multi(src_d, blobs, ns, want_indices=True)
        midx = midx[None]
    else:                        # M = 2, a negative weight too
        w = torch.tensor([[0.7, 0.3], [1.2, -0.2], [0.5, 0.5]], device=DEV)
        blobs, ns = prepare_references([targets[(b + m) % 4] for b in range(B) for m in range(2)])
        mu, midx = eng.knn_match_blend(src_d, blobs, ns, w, want_indices=True)
    weights = torch.stack([frame_weights(f0[b]) for b in range(B)])
    assert set(weights[0].tolist()) == {0.0, 0.25, 0.75, 1.0} and (weights[2] == 1).all()
    for alphas, protects in STAGE_SETS:
        a, p = torch.tensor(alphas, device=DEV), torch.tensor(protects, device=DEV)
        out, idx = eng.knn_match_protect(src_d, f0_d, blobs, ns, a, p, weights=w, want_indices=True)
        a_t = torch.stack([frame_share(f0_d[b], a[b], p[b]) for b in range(B)]).view(B, 1, T)
        assert torch.equal(out, mu * (1 - a_t) + src_d * a_t), f"{form} {alphas} {protects}: not the bits of torch's mu * (1 - a_t) + src * a_t"
        assert idx.shape == midx.shape and torch.equal(idx, midx), f"{form}: the indices depend on protect"
        for b in range(B):
            if alphas[b] == 0.0 and protects[b] == 1.0:
                full, none = weights[b] == 1, weights[b] == 0
                assert full.any() and torch.equal(out[b][:, full], src_d[b][:, full]), f"{form}: a = 0, p = 1, w = 1 must carry the source's bits"
                assert torch.equal(out[b][:, none], mu[b][:, none]), f"{form}: a = 0, w = 0 must carry the alpha-less bits"
        # protect 0 is the alpha call; alpha None is alpha 0
        assert torch.equal(eng.knn_match_protect(src_d, f0_d, blobs, ns, a, torch.zeros(B, device=DEV), weights=w),
                           eng.knn_match_alpha(src_d, blobs, ns, a, weights=w)), f"{form} {alphas}: protect = 0 is not knn_match_alpha"
    p = torch.tensor(STAGE_SETS[0][1], device=DEV)
    assert torch.equal(eng.knn_match_protect(src_d, f0_d, blobs, ns, None, p, weights=w),
                       eng.knn_match_protect(src_d, f0_d, blobs, ns, torch.zeros(B, device=DEV), p, weights=w))


# ---- 3. the fused conversion, equal lengths --------------------------------------------------------------------------------------------
B2, T2 = 2, 100
SHIFTS2, ALPHAS2, PROTECTS2 = [2.0, -3.0], [0.3, 0.0], [0.5, 1.0]
UNVOICED2 = [range(1, 18), range(1, 12)]      # what the CPU oracle finds on the case below: 17 and 11 unvoiced frames of 100, frame 0 voiced


def _equal_case(scale=1.0):
    wf = synth.synth_wave(B2, T2 * 480, seed=41) * scale
    return wf, synth.synth_angle(B2, T2, 42).to(DEV)


def _oracle_protect_convert(enc_sd, dec_sd, wf, ref, alpha, protect, shift, angle):
    """the reference's convert with the definition between its match (alpha 0) and its decoder"""
    with torch.inference_mode():
        wf = R.autopad_waveform(wf)
        spec = R.spectrogram(wf)
        energy = R.estimate_energy(wf)
        z, f0 = R.encoder_infer(enc_sd, spec)
        mu = R.match_features(z, ref, alpha=0.0)
        a_t = frame_share(f0[0, 0], alpha, protect).view(1, 1, -1)
        return R.decoder_infer(dec_sd, mu * (1 - a_t) + z * a_t, R.shift_frequency(f0, shift), energy, angle), f0


def test_convert_equal_lengths(gen, targets):
    enc_sd, dec_sd = state_dicts(0)
    wf, angle = _equal_case()
    tg = [targets[1], targets[2]]
    # the precondition, naming the input: the device's voicing flags on this case are the oracle's
    _, f0_dev = gen.encode(wf.to(DEV))
    for b in range(B2):
        unvoiced = (~(f0_dev[b, 0] > 0)).nonzero().flatten().tolist()
        assert unvoiced == list(UNVOICED2[b]), f"row {b}: the device finds unvoiced frames {unvoiced}"
    out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=PROTECTS2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b], protect=PROTECTS2[b])
        assert torch.equal(out[b:b + 1], one), f"row {b}: the batched protect call != its B = 1 call"
        with oracle_one_thread():
            ref, f0 = _oracle_protect_convert(enc_sd, dec_sd, wf[b:b + 1], tg[b].float().cpu(), ALPHAS2[b], PROTECTS2[b], SHIFTS2[b], angle[b:b + 1].cpu())
        assert (~(f0[0, 0] > 0)).nonzero().flatten().tolist() == list(UNVOICED2[b])
        d = rms(out[b].cpu() - ref[0])
        print(f"[protect] row {b}: {d:.3e} rms vs the oracle composition")
        assert d <= 1e-4, f"row {b}: {d:.3e} rms vs the oracle composition"
    only_alpha = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2)
    assert not torch.equal(out[0], only_alpha[0]) and not torch.equal(out[1], only_alpha[1]), "protect changed nothing"
    # protect 0: the alpha call bit for bit, as a float and as a device tensor used in place; without alpha too: the plain call
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=0.0), only_alpha)
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=torch.zeros(B2, device=DEV)), only_alpha)
    plain = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle)
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, protect=0.0), plain)
    # alpha None is alpha 0
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, protect=PROTECTS2),
                       gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=0.0, protect=PROTECTS2))
    # one shared index and one shift take the same entry
    shared = gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, alpha=0.3, protect=PROTECTS2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), targets[1], 1.0, noise_angle=angle[b:b + 1].contiguous(), alpha=0.3, protect=PROTECTS2[b])
        assert torch.equal(shared[b:b + 1], one), f"row {b}: the shared-index protect call != its B = 1 call"
    assert torch.equal(gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, protect=[0.0, 0.0]), gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle))
    # a blend target
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    blend = Blend([[targets[0], targets[1]], [targets[2], targets[3]]], torch.tensor([[0.7, 0.3], [0.25, 0.75]], device=DEV))
    ob = gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=PROTECTS2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), Blend([blend.terms[0][b], blend.terms[1][b]], blend.weights[b].tolist()), SHIFTS2[b],
                          noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b], protect=PROTECTS2[b])
        assert torch.equal(ob[b:b + 1], one), f"row {b}: the batched protect blend != its B = 1 call"
    assert torch.equal(gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=0.0),
                       gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, alpha=ALPHAS2))


def test_convert_auto_pitch_shifts_do_not_depend_on_protect(gen, targets):
    wf, angle = _equal_case()
    tg = [targets[1], targets[2]]
    reg = torch.tensor([180.0, 240.0], device=DEV)
    base, sh0 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, alpha=ALPHAS2)
    out, sh = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, alpha=ALPHAS2, protect=PROTECTS2)
    assert torch.equal(sh, sh0), "the shifts found on the device depend on protect"
    assert not torch.equal(out, base) and torch.isfinite(out).all()
    zero, shz = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, alpha=ALPHAS2, protect=0.0)
    assert torch.equal(zero, base) and torch.equal(shz, sh0)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), auto_pitch=reg[b:b + 1].contiguous(),
                          alpha=ALPHAS2[b], protect=PROTECTS2[b])
        assert torch.equal(out[b:b + 1], one), f"row {b}: the batched auto-pitch protect call != its B = 1 call"


# ---- 4. ragged batches -----------------------------------------------------------------------------------------------------------------
def test_convert_ragged(gen, targets):
    """test_gpu_alpha.py::test_convert_ragged's frames - one row per length class, then eight rows under a frame cap that cuts the two upper
    classes into two in-kernel batches each - with an alpha and a protect of its own in every row: each row equals its own B = 1 call over its
    own length (its neighbours in the packed batch never reach its edge frames)."""
    frames = [7, 150, 33, 60, 9, 131, 20, 90]
    lens = [480 * f - (11 if i % 2 else 0) for i, f in enumerate(frames)]
    alphas = [0.3, 1.25, 0.0, -0.4, 1.0, 0.5, 0.8, 0.05]
    protects = [1.0, 0.5, 0.75, 1.0, 0.5, 0.0, 0.25, 1.0]
    B, Lmax, Tmax = len(frames), 480 * max(frames), max(frames)
    wf = torch.zeros(B, Lmax)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=600 + b)[0]
    mixed = 0
    for b in range(B):
        voiced = gen.encode(wf[b:b + 1, :lens[b]].to(DEV))[1][0, 0] > 0
        mixed += bool(voiced.any() and not voiced.all())
    assert mixed >= 1, "no row holds both voiced and unvoiced frames: the case does not reach the per-frame share"
    tg = [targets[b % 4] for b in range(B)]
    angle = synth.synth_angle(B, Tmax, 61).to(DEV)
    ones = [gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tg[b], -2.0, noise_angle=angle[b:b + 1, :, :f].contiguous(), alpha=alphas[b], protect=protects[b])
            for b, f in enumerate(frames)]
    eng = gen.engine()
    try:
        for rows, cap in ((4, 0), (4, 100), (8, 100)):
            eng.set_ragged_batch_frames(cap)
            a, p = torch.tensor(alphas[:rows], device=DEV), torch.tensor(protects[:rows], device=DEV)
            out = gen.convert(wf[:rows].to(DEV), tg[:rows], -2.0, noise_angle=angle[:rows].contiguous(), lengths=lens[:rows], alpha=a, protect=p)
            for b in range(rows):
                f = frames[b]
                assert torch.equal(out[b, :480 * f], ones[b][0]), f"{rows} rows, cap {cap}: row {b} ({f} frames, alpha {alphas[b]}, protect {protects[b]})"
                assert not out[b, 480 * f:].any()
    finally:
        eng.set_ragged_batch_frames(0)


# ---- 5. the range guard ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e4, 1e-7])
def test_range_guard(gen, targets, scale):
    """the equal-length case at two input amplitudes: the content bound follows max(|a|, |a_u|) times the source's own |max|"""
    wf, angle = _equal_case(scale)
    tg = [targets[1], targets[2]]
    out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, alpha=ALPHAS2, protect=PROTECTS2)
    assert torch.isfinite(out).all()
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), alpha=ALPHAS2[b], protect=PROTECTS2[b])
        assert torch.equal(out[b:b + 1], one), f"scale {scale}: row {b} != its B = 1 call"


# ---- 6. streams ------------------------------------------------------------------------------------------------------------------------
def test_streams_follow_live_protect_without_a_new_capture(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk = 2, 8
    tg = [targets[0], synth.synth_index(800, seed=83).to(DEV)]
    p0, new = [0.5, 1.0], torch.tensor([1.0, 0.25])
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)
    sts = {}
    for use_graph in (True, False):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840,
                                use_graph=use_graph, protect=p0)
        st.init_buffer()
        assert st.alpha is None and st.protect.shape == (S,) and st.protect.dtype == torch.float32 and st.protect.device == torch.device(DEV)
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
        sts[g].protect.copy_(new)                                # the knob moves: in place, on the device
    for i in range(4, nblk):
        a, b = block(i)
        assert torch.equal(a, b), f"block {i + 1}: the replay did not follow the new protect"
        assert sts[True]._graph[1][True][0] is graph3, "changing protect in place must not capture again"
    # and the knob does something: the same blocks without protect differ (the window's first frames are silence: unvoiced)
    st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840)
    st.init_buffer()
    assert st.protect is None
    ys = [st.audio_callback(blocks[:, i], noise_angle=synth.synth_angle(S, st.input_size // 480, 850 + i).to(DEV)).clone() for i in range(4)]
    assert any(not torch.equal(y, o) for y, o in zip(ys, outs))


def test_stream_with_tracker_door_and_alpha_in_one_graph(gen, targets):
    """protect beside alpha, a live pitch tracker and a door at 48 kHz: one captured block, equal to the eager stream block for block"""
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor
    S, nblk = 2, 6
    tg = [targets[0], targets[1]]
    sts = {}
    for use_graph in (True, False):
        door = StreamDoor(S, 48000, block_size=1920, device=DEV)
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=0.5, device=torch.device(DEV), block_size=1920, extra_size=3840, use_graph=use_graph,
                                door=door, auto_pitch=torch.tensor([200.0, 150.0], device=DEV), alpha=[0.4, 0.0], protect=[0.5, 1.0])
        st.init_buffer()
        sts[use_graph] = st
    chunk = sts[True].door.chunk_in
    pcm = (synth.synth_wave(S, nblk * chunk, seed=91) * 20000).clamp(-32768, 32767).to(torch.int16).view(S, nblk, chunk).to(DEV)
    for i in range(nblk):
        if i == 4:
            for g in (True, False):
                sts[g].protect.fill_(0.75)
        angle = synth.synth_angle(S, sts[True].input_size // 480, 950 + i).to(DEV)
        a, b = [sts[g].audio_callback_pcm(pcm[:, i], noise_angle=angle).clone() for g in (True, False)]
        assert a.dtype == torch.int16 and torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(sts[True].last_pitch_shift, sts[False].last_pitch_shift)
    assert len(sts[True]._graph[1]) == 1, "one captured block"


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(gen, targets, src):
    """a protect the entries cannot take is refused on the host, under its name, before anything is launched"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    B, _, T = src.shape
    src_d, f0_d = src.to(DEV), _stage_f0().to(DEV)
    blobs, ns = prepare_references([targets[0]] * B)
    a = torch.zeros(B, device=DEV)
    for bad, exc in ((torch.zeros(B + 1, device=DEV), ValueError), (torch.zeros(B, dtype=torch.float64, device=DEV), ValueError),
                     (torch.zeros(B, 1, device=DEV), ValueError), (torch.zeros(B), RuntimeError), ([0.0] * B, TypeError), (0.5, TypeError)):
        with pytest.raises(exc, match="protect"):
            eng.knn_match_protect(src_d, f0_d, blobs, ns, a, bad)
        with pytest.raises(exc, match="protect"):
            eng.frame_share(f0_d, [0, 45, 90], [45, 45, 45], a, bad)
    with pytest.raises(ValueError, match="f0"):
        eng.knn_match_protect(src_d, f0_d[:, :44].contiguous(), blobs, ns, a, a)
    with pytest.raises(ValueError, match="frame_share"):
        eng.frame_share(f0_d, [0, 100], [45, 45], a[:2].contiguous(), a[:2].contiguous())
    wf = synth.synth_wave(2, 9600, seed=1).to(DEV)
    angle = synth.synth_angle(2, 20, 3).to(DEV)
    before = torch.cuda.get_rng_state(DEV).clone()
    for bad in (torch.zeros(2), torch.zeros(3, device=DEV), torch.zeros(2, dtype=torch.float16, device=DEV), [0.1, 0.2, 0.3], "0.5", True):
        with pytest.raises(ValueError, match="protect"):
            gen.convert(wf, targets[0], 0.0, noise_angle=angle, protect=bad)
        with pytest.raises(ValueError, match="protect"):
            gen.convert(wf, targets[0], 0.0, alpha=0.5, protect=bad)      # refused before the noise draw
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)
