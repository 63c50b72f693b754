"""Weighted neighbours in the fused match: a k of 1 .. 4 and a similarity width per row (tvc_knn_match_weighted_f32, tvc_weighted_convert_f32,
tvc_weighted_convert_ragged_f32; Engine.knn_match_weighted, Generator.convert(k=, match_width=), BatchedStreamInfer(k=, match_width=)).

Contract (include/tinyvc_hip.h): with s_0 >= .. >= s_3 and i_0 .. i_3 the merged top-4 of a query column of row r - what every other entry
selects -, k = clamp(neighbours[r], 1, 4) and w_e = clamp(1 - (s_0 - s_e) / width[r], 0, 1) (1 wherever that quotient is not a positive
number, 0 from k on), the column's matched value is (r_0 + w_1 r_1 + ..) / (w_0 + ..), every operation one fp32 rounding.
tests/helpers_match_weight.py restates it in numpy; the outputs here equal it bit for bit when it is evaluated from the call's OWN sims_out
and idx_out, and sims_out itself is held against the fp64 cosine within 770 * 2^-24, the fp32 accumulation bound of a 768-term product of
unit vectors (derived, not measured; the measured maximum on an MI355X over these shapes is 9.9e-7, the figure the README paragraph gives)."""
import numpy as np
import pytest
import torch

import helpers_match_weight as mw
import helpers_workspace as W
from helpers import state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
INF = float("inf")
SIM_TOL = 770 * 2.0 ** -24
WIDTHS = [INF, 0.02, 0.005, 0.0]
KS = [[1, 2, 3], [4, 3, 2], [2, 4, 1], [3, 1, 4]]      # k of 1 .. 4 mixed across the rows, call by call


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
    """test_gpu_alpha.py's: B = 3, T = 45 - 135 query columns, the 32-column tiles straddle the row edges at 45 and 90, the last holds 7"""
    return torch.randn(3, 768, 45, generator=torch.Generator().manual_seed(5))


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _rows(t):
    """an index tensor [1, 768, N] (fp32 or fp16) -> the rows the gather reads, [N, 768] fp32 on the host"""
    return t[0].float().t().contiguous().cpu().numpy()


def _ints(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _floats(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def near_source(terms, T=45, seed=11):
    """Queries whose four nearest rows lie CLOSE together, so that the widths 0.02 and 0.005 reach the inside of the ramp: terms[b] = the
    index tensors row b searches (one, or a blend's M).  Column t of row b is the minimum-norm vector whose inner products with four chosen
    unit rows of each term are 0.5 * (1 - e * d_t), d_t uniform in [0, 0.02]: the cosine gaps between neighbours run from 0 to a few
    hundredths, without ties.  -> [B, 768, T] fp32"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(terms), 768, T), F)
    for b, ts in enumerate(terms):
        rows = [_rows(t).astype(np.float64) for t in ts]
        for t in range(T):
            d = rng.uniform(0, 0.02)
            Rm = np.concatenate([r[rng.choice(len(r), 4, replace=False)] for r in rows])
            Rm /= np.linalg.norm(Rm, axis=1, keepdims=True)
            s = np.tile(0.5 * (1 - d * np.arange(4)), len(rows))
            out[b, :, t] = (Rm.T @ np.linalg.solve(Rm @ Rm.T, s)).astype(F)
    return torch.from_numpy(out)


FORMS = {      # form -> (row b's terms as positions in `targets`, blend weights or None)
    "table": ([[0], [1], [3]], None),                                        # the exact kernel and the two-stage search in one call
    "fp16": ([[2], [2], [2]], None),                                         # one fp16-kind blob in every row
    "blend": ([[0, 1], [1, 2], [2, 3]], [[0.7, 0.3], [1.2, -0.2], [0.5, 0.5]]),      # M = 2, a negative weight too
}


def _form(targets, form):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    pos, w = FORMS[form]
    terms = [[targets[p] for p in row] for row in pos]
    blobs, ns = prepare_references([t for row in terms for t in row])
    return terms, blobs, ns, (_floats(w) if w is not None else None)


def restate(src, terms, sims, idx, k, width, weights=None, share=None):
    """the definition from the call's own lists: src [B, 768, T], terms[b][m] index tensors, sims / idx [M, B, T, 4], k / width one per row,
    weights [B, M] (a blend) or None, share [B, T] (the source's share of every column: alpha, or protect's a_t) or None -> out [B, 768, T]"""
    src = src.cpu().numpy()
    sims, idx = sims.cpu().numpy(), idx.cpu().numpy()
    B, _, T = src.shape
    out = np.zeros_like(src)
    for b in range(B):
        acc = None
        for m, t in enumerate(terms[b]):
            mu = mw.match(sims[m, b], idx[m, b], _rows(t), k[b], width[b])      # [T, 768]
            if weights is not None:
                term = (F(weights[b][m]) * mu).astype(F)
                acc = term if acc is None else (acc + term).astype(F)
            else:
                acc = mu
        acc = acc.T
        if share is not None:
            a = share[b].astype(F)[None, :]
            acc = ((acc * (F(1) - a).astype(F)).astype(F) + (src[b] * a).astype(F)).astype(F)
        out[b] = acc
    return torch.from_numpy(out)


# ---- 1. the similarities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_similarities_are_the_cosines(targets, src, form):
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    worst = 0.0
    for s in (src, near_source(terms)):
        _out, idx, sims = eng.knn_match_weighted(s.to(DEV), blobs, ns, weights=w, want_indices=True, want_similarities=True)
        assert sims.shape == idx.shape == (len(terms[0]), 3, 45, 4) and sims.dtype == torch.float32
        q = s.double().numpy()
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        for b in range(3):
            for m, t in enumerate(terms[b]):
                r = _rows(t).astype(np.float64)[idx[m, b].cpu().numpy()]                      # [T, 4, 768]
                cos = np.einsum("tec,ct->te", r / np.linalg.norm(r, axis=2, keepdims=True), q[b])
                worst = max(worst, float(np.abs(sims[m, b].cpu().numpy().astype(np.float64) - cos).max()))
        assert bool((sims[..., :-1] >= sims[..., 1:]).all()), "the lists are not sorted"
    print(f"[match_weight] {form}: max |sims_out - fp64 cosine| = {worst:.3e} (bound {SIM_TOL:.3e})")
    assert worst <= SIM_TOL, (form, worst)


# ---- 2. the bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["plain", "alpha", "protect"])
@pytest.mark.parametrize("form", list(FORMS))
def test_stage_bits(targets, form, mix):
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    s = near_source(terms)
    s_d = s.to(DEV)
    B, _, T = s.shape
    _mu, plain_idx = (eng.knn_match_blend(s_d, blobs, ns, w, want_indices=True) if w is not None else eng.knn_match_multi(s_d, blobs, ns, want_indices=True))
    plain_idx = plain_idx if w is not None else plain_idx[None]
    kw, share = {}, None
    if mix != "plain":
        kw["alpha"] = _floats([0.0, 0.35, 1.5])
        share = np.repeat(np.array([0.0, 0.35, 1.5], F)[:, None], T, axis=1)
    if mix == "protect":      # a planted f0: voiced runs, single unvoiced frames, an unvoiced edge, a NaN
        f0 = torch.full((B, T), 150.0)
        f0[0, :7] = 0.0
        f0[1, 10::3] = 0.0
        f0[2, 20:30] = -1.0
        f0[2, 44] = float("nan")
        kw["f0"], kw["protect"] = f0.to(DEV), _floats([0.5, 1.0, 0.25])
        share = eng.frame_share(kw["f0"], [b * T for b in range(B)], [T] * B, kw["alpha"], kw["protect"]).cpu().numpy()
    seen = {}
    for j, ks in enumerate(KS):
        widths = [WIDTHS[(j + b) % 4] for b in range(B)]
        out, idx, sims = eng.knn_match_weighted(s_d, blobs, ns, _ints(ks), _floats(widths), weights=w, want_indices=True, want_similarities=True, **kw)
        assert torch.equal(idx, plain_idx), f"{form} {mix} call {j}: the indices depend on neighbours / width"
        want = restate(s, terms, sims, idx, ks, widths, FORMS[form][1], share)
        assert W.same_bits(out.cpu(), want), f"{form} {mix} k {ks} widths {widths}: {W.first_difference(out.cpu(), want)}"
        seen["sims"] = sims.cpu().numpy()
    # the condition on the inputs: each finite non-zero width reaches the inside of the ramp on a quarter of the (column, neighbour) weights
    # at least, and its end on one at least (chosen on the CPU with the oracle's similarities; held here on the call's own)
    for width in (0.02, 0.005):
        wts, _ = mw.weights(seen["sims"], 4, width)
        inside = float(((wts[..., 1:] > 0) & (wts[..., 1:] < 1)).mean())
        print(f"[match_weight] {form}: width {width}: {inside:.2f} of the weights inside (0, 1), {int((wts == 0).sum())} at 0")
        assert inside >= 0.25 and (wts == 0).any(), (form, width, inside)


# ---- 3. off is off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_off_is_off(targets, src, form):
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    s_d = src.to(DEV)
    a, p = _floats([0.0, 0.35, 1.5]), _floats([0.5, 1.0, 0.25])
    f0 = torch.full((3, 45), 150.0)
    f0[:, ::4] = 0.0
    f0 = f0.to(DEV)
    siblings = {"plain": (eng.knn_match_blend(s_d, blobs, ns, w) if w is not None else eng.knn_match_multi(s_d, blobs, ns), {}),
                "alpha": (eng.knn_match_alpha(s_d, blobs, ns, a, weights=w), dict(alpha=a)),
                "protect": (eng.knn_match_protect(s_d, f0, blobs, ns, a, p, weights=w), dict(alpha=a, protect=p, f0=f0))}
    for name, (want, kw) in siblings.items():
        assert torch.equal(eng.knn_match_weighted(s_d, blobs, ns, weights=w, **kw), want), f"{form} {name}: both NULL is not the sibling call"
        assert torch.equal(eng.knn_match_weighted(s_d, blobs, ns, _ints([4] * 3), _floats([INF] * 3), weights=w, **kw), want), f"{form} {name}: (4, inf)"
        assert torch.equal(eng.knn_match_weighted(s_d, blobs, ns, None, _floats([INF] * 3), weights=w, **kw), want), f"{form} {name}: (NULL, inf)"
        assert torch.equal(eng.knn_match_weighted(s_d, blobs, ns, _ints([4] * 3), None, weights=w, **kw), want), f"{form} {name}: (4, NULL)"
    plain = siblings["plain"][0]
    if w is None:      # k = 1: the gathered nearest rows, bit for bit (-0.0 and all)
        out, idx = eng.knn_match_weighted(s_d, blobs, ns, _ints([1] * 3), want_indices=True)
        for b in range(3):
            nearest = torch.from_numpy(_rows(terms[b][0])[idx[0, b, :, 0].cpu().numpy()].T.copy())
            assert W.same_bits(out[b].cpu(), nearest), f"{form}: row {b}: k = 1 is not the nearest row"
        assert W.same_bits(eng.knn_match_weighted(s_d, blobs, ns, None, _floats([0.0] * 3)).cpu(), out.cpu()), f"{form}: width 0 without ties"
    # garbage in the two arrays: k of -7 and 1 000 are 1 and 4, widths NaN and -1 are uniform - features, no error
    out, idx, sims = eng.knn_match_weighted(s_d, blobs, ns, _ints([-7, 1000, 2]), _floats([float("nan"), -1.0, float("nan")]), weights=w, want_indices=True,
                                            want_similarities=True)
    want = restate(src, terms, sims, idx, [1, 4, 2], [INF] * 3, FORMS[form][1])
    assert W.same_bits(out.cpu(), want), f"{form}: garbage: {W.first_difference(out.cpu(), want)}"
    if w is None:
        assert torch.equal(out[1], plain[1]), f"{form}: k = 1000 under width -1 is not the plain row"


# ---- 4. the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_stage_against_the_oracle(targets, src):
    """oracle.ref_cpu.match_features(..., k=) for k = 1, 2, 3 against the 6 000-vector index, whose top-5 gaps against this source are above
    1e-5 (test_gpu_alpha.py): indices equal, the output within that test's 2e-7 of the output's |max|"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    ref = targets[1]
    blobs, ns = prepare_references([ref] * 3)
    ks = [1, 2, 3]
    out, idx = eng.knn_match_weighted(src.to(DEV), blobs, ns, _ints(ks), want_indices=True)
    for b, k in enumerate(ks):
        want, o_idx, sims = R.match_features(src[b:b + 1], ref.cpu(), k=k, return_indices=True)
        top = torch.topk(sims.double(), 5, dim=2).values
        assert float((top[..., :-1] - top[..., 1:]).min()) > 1e-5, "the oracle alone cannot decide this index"
        assert torch.equal(idx[0, b, :, :k].cpu(), o_idx[0]), f"row {b}: the first {k} indices differ from the oracle's"
        err = float((out[b:b + 1].cpu() - want).abs().max() / want.abs().max())
        print(f"[match_weight] row {b} k {k}: {err:.2e} of the output's |max| vs the oracle")
        assert err <= 2e-7, (b, k, err)


# ---- 5. the fused conversion -----------------------------------------------------------------------------------------------------------------
B2, T2 = 2, 28
SHIFTS2 = [2.0, -3.0]
K2, WIDTH2 = [2, 3], [0.02, 0.005]


def _stages(gen, wf):
    from tinyvc_amd.module import utils
    eng = gen.engine()
    w = utils.autopad_waveform(wf.to(DEV))
    ssl, f0, logits = eng.encoder(utils.spectrogram(w), want_logits=True)
    return eng, ssl, f0, logits, utils.estimate_energy(w)


def test_convert_equals_its_stage_composition(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, f0, _logits, energy = _stages(gen, wf)
    tg = [targets[1], targets[2]]
    blobs, ns = prepare_references(tg)
    f0s = eng.pitch_match(f0, pitch_shift=SHIFTS2, want_shifted=True)[3]
    plain = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle)
    assert torch.equal(plain, eng.decoder(eng.knn_match_multi(ssl, blobs, ns), f0s, energy, angle)), "the composition is not today's call: the comparison shows nothing"
    for kw, mkw in ((dict(k=K2, match_width=WIDTH2), dict(neighbours=_ints(K2), width=_floats(WIDTH2))),
                    (dict(k=1), dict(neighbours=_ints([1, 1]))),
                    (dict(match_width=_floats([0.01, 0.0])), dict(width=_floats([0.01, 0.0]))),
                    (dict(k=_ints([3, 2]), match_width=0.02, alpha=[0.3, 0.0]), dict(neighbours=_ints([3, 2]), width=_floats([0.02] * 2), alpha=_floats([0.3, 0.0])))):
        out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, **kw)
        matched = eng.knn_match_weighted(ssl, blobs, ns, **mkw)
        assert torch.equal(out, eng.decoder(matched, f0s, energy, angle)), f"{kw}: convert != the stages, knn_match_weighted, the decoder"
        assert not torch.equal(out, plain), f"{kw}: the weights changed nothing"
        for b in range(B2):      # a row equals its own call (each row has a blob, and so a segment of the search, of its own)
            one = {n: (v[b:b + 1].contiguous() if isinstance(v, torch.Tensor) else v[b] if isinstance(v, list) else v) for n, v in kw.items()}
            y = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), **one)
            assert torch.equal(out[b:b + 1], y), f"{kw}: row {b} != its own B = 1 call"
    # off is off: k = 4 under an infinite width, as host values and as device tensors; one shared index takes the same entry
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, k=4, match_width=INF), plain)
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, k=_ints([4, 4]), match_width=_floats([INF, INF])), plain)
    shared = gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle)
    assert torch.equal(gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, k=[4, 4]), shared)
    assert not torch.equal(gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, k=[4, 1]), shared)
    # a blend target: every term's match is weighted, row by row its own call
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    blend = Blend([[targets[0], targets[1]], [targets[2], targets[3]]], torch.tensor([[0.7, 0.3], [0.25, 0.75]], device=DEV))
    ob = gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), Blend([blend.terms[0][b], blend.terms[1][b]], blend.weights[b].tolist()), SHIFTS2[b],
                          noise_angle=angle[b:b + 1].contiguous(), k=K2[b], match_width=WIDTH2[b])
        assert torch.equal(ob[b:b + 1], one), f"row {b}: the batched weighted blend != its B = 1 call"
    assert torch.equal(gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, k=4), gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle))


def test_convert_with_every_other_keyword(gen, targets):
    """tune, the pitch path and auto_pitch beside the weights: (4, inf) is the call without them, the weighted call differs from it and
    every row equals its own B = 1 call"""
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    tg = [targets[1], targets[2]]
    reg = torch.tensor([180.0, 240.0], device=DEV)
    kw = dict(tune="chromatic", f0_estimation="viterbi", protect=[0.5, 1.0])
    plain, sh0 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, **kw)
    same, sh1 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, k=4, match_width=INF, **kw)
    assert torch.equal(same, plain) and torch.equal(sh1, sh0)
    out, sh = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, k=K2, match_width=WIDTH2, **kw)
    assert torch.equal(sh, sh0), "the shifts found on the device depend on the weights"
    assert torch.isfinite(out).all() and not torch.equal(out, plain)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), auto_pitch=reg[b:b + 1].contiguous(), k=K2[b],
                          match_width=WIDTH2[b], tune="chromatic", f0_estimation="viterbi", protect=kw["protect"][b])
        assert torch.equal(out[b:b + 1], one), f"row {b} != its own B = 1 call"


def test_convert_ragged(gen, targets):
    """a ragged pair, 28 and 21 frames: each row equals the stage composition over its own length, with its own k and width"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    frames = [28, 21]
    lens = [f * 480 for f in frames]
    wf = synth.synth_wave(2, 28 * 480, seed=51)
    wf[1, lens[1]:] = 0
    tg = [targets[1], targets[0]]
    angle = synth.synth_angle(2, 28, 61).to(DEV)
    out = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, k=K2, match_width=_floats(WIDTH2))
    today = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens)
    assert torch.equal(gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, k=4, match_width=INF), today)
    assert not torch.equal(out, today)
    blobs, ns = prepare_references(tg)
    for b, f in enumerate(frames):
        eng, ssl, f0, _logits, energy = _stages(gen, wf[b:b + 1, :lens[b]])
        matched = eng.knn_match_weighted(ssl, blobs[b:b + 1], ns[b:b + 1], _ints(K2[b:b + 1]), _floats(WIDTH2[b:b + 1]))
        want = eng.decoder(matched, eng.shift_frequency(f0, -2.0), energy, angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b:b + 1, :lens[b]], want), f"row {b} of {f} frames != its own stage composition"
        assert not out[b, lens[b]:].any()
        one = gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tg[b], -2.0, noise_angle=angle[b:b + 1, :, :f].contiguous(), k=K2[b], match_width=WIDTH2[b])
        assert torch.equal(out[b:b + 1, :lens[b]], one), f"row {b} != its own B = 1 call"


# ---- 6. streams ------------------------------------------------------------------------------------------------------------------------------
def test_streams_follow_live_k_and_width_without_a_new_capture(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk = 2, 6
    tg = [targets[0], synth.synth_index(800, seed=83).to(DEV)]
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)

    def make(use_graph, k=(3, 2), width=(0.02, INF)):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840,
                                use_graph=use_graph, k=list(k), match_width=list(width))
        st.init_buffer()
        assert st.k.shape == (S,) and st.k.dtype == torch.int32 and st.match_width.shape == (S,) and st.match_width.dtype == torch.float32
        return st

    sts = {True: make(True), False: make(False)}
    other = make(False, k=(3, 4), width=(0.02, 0.001))      # stream 1 differs: stream 0 must not notice

    def block(i):
        angle = synth.synth_angle(S, sts[True].input_size // 480, 850 + i).to(DEV)
        return [st.audio_callback(blocks[:, i], noise_angle=angle).clone() for st in (sts[True], sts[False], other)]

    for i in range(3):
        a, b, c = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(a[0], c[0]), f"block {i + 1}: stream 0 depends on stream 1's k / width"
        assert not torch.equal(a[1], c[1]), f"block {i + 1}: stream 1's k / width changed nothing"
    graph3 = sts[True]._graph[1][True][0]                        # captured at block 3
    for st in (sts[True], sts[False], other):                    # the knobs move: in place, on the device
        st.k.fill_(1)
        st.match_width.fill_(0.003)
    still = make(False)                                          # the same stream left at its first values
    for i in range(3):
        still.audio_callback(blocks[:, i], noise_angle=synth.synth_angle(S, still.input_size // 480, 850 + i).to(DEV))
    for i in range(3, nblk):
        a, b, c = block(i)
        assert torch.equal(a, b), f"block {i + 1}: the replay did not follow the new k / width"
        assert sts[True]._graph[1][True][0] is graph3, "changing k / match_width in place must not capture again"
        y = still.audio_callback(blocks[:, i], noise_angle=synth.synth_angle(S, still.input_size // 480, 850 + i).to(DEV))
        assert not torch.equal(a, y), f"block {i + 1}: fill_ between replays took no effect"
    # a stream without the keywords is the stream as it was
    st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840)
    st.init_buffer()
    assert st.k is None and st.match_width is None


# ---- 7. the workspace ------------------------------------------------------------------------------------------------------------------------
def _poisoned(name, eng, call, tight=False):
    """tests/helpers_workspace.py's scheme: the call in a guarded workspace of exactly its peak under every fill word equals the call as it is"""
    want = call()
    torch.cuda.synchronize()
    peak = W.exact_peak(eng, call) if tight else None
    assert not tight or peak is not None, f"{name}: the zero-byte probe was not refused"
    for word, phase in zip(W.FILLS, W.PHASES):
        with W.guarded_workspace(eng, word, phase, peak=peak) as g:
            got = call()
        W.assert_same_bits(got, want, f"{name} under fill {word:#010x} at phase {phase}")
    print(f"[match_weight] {name}: carved peak {'+'.join(str(p) for p in g.peaks)} bytes, {len(W.FILLS)} fills passed")


def test_the_existing_queries_suffice_in_a_poisoned_workspace(gen, targets, src):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath, PitchSnap, prepare_references
    eng = gen.engine()
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41).to(DEV), synth.synth_angle(B2, T2, 42).to(DEV)
    blobs, ns = prepare_references([targets[1], targets[2]])
    k, width, a, p = _ints(K2), _floats(WIDTH2), _floats([0.25, 0.6]), _floats([0.5, 1.0])
    reg = _floats([150.0, 220.0])

    def tune():
        return PitchSnap(scale="chromatic", low=12, retune_ms=40.0, strength=[1.0, 0.5])

    _poisoned("weighted convert", eng, lambda: eng._convert("weighted", wf, blobs, ns, SHIFTS2, angle, None, None, reg, alpha=a, protect=p, path=PitchPath(),
                                                             tune=tune(), neighbours=k, width=width))
    lens = [28 * 480, 21 * 480]
    rag = wf.clone()
    rag[1, lens[1]:] = 0
    _poisoned("weighted convert_ragged", eng, lambda: eng._convert("weighted", rag, blobs, ns, SHIFTS2, angle, lens, None, reg, alpha=a, protect=p, path=PitchPath(),
                                                                    tune=tune(), neighbours=k, width=width))
    s_d = src[:2].contiguous().to(DEV)
    f0 = torch.full((2, 45), 150.0)
    f0[:, ::4] = 0.0
    f0 = f0.to(DEV)
    _poisoned("knn_match_weighted", eng, lambda: eng.knn_match_weighted(s_d, blobs, ns, k, width, alpha=a, f0=f0, protect=p, want_indices=True,
                                                                        want_similarities=True), tight=True)


# ---- 8. the point ----------------------------------------------------------------------------------------------------------------------------
def test_the_point_a_planted_row_comes_back_whole():
    """the index holds row A, the query is A plus small noise, the three other neighbours lie near 0.3 cosine: the plain call blurs A with
    them, width 0.1 and k = 1 return A's bits"""
    eng = _engine()
    rows, q, a = mw.planted_index()
    index = torch.from_numpy(rows.T.copy())[None].to(DEV)
    blob, n = eng.knn_prepare(index)
    s_d = torch.from_numpy(np.repeat(q[None, :, None], 5, axis=2).copy()).to(DEV)      # [1, 768, 5]: the query in every column
    A = torch.from_numpy(np.repeat(rows[a][:, None], 5, axis=1).copy())
    plain, idx = eng.knn_match_multi(s_d, [blob], [n], want_indices=True)
    assert bool((idx[0, :, 0] == a).all()) and sorted(idx[0, 0, 1:].tolist()) == [40, 41, 42]
    assert float((plain[0].cpu() - A).norm(dim=0).min()) > 0.5, "the flat mean of four should have lost most of A"
    for kw in (dict(width=_floats([0.1])), dict(neighbours=_ints([1]))):
        out = eng.knn_match_weighted(s_d, [blob], [n], **kw)
        assert W.same_bits(out[0].cpu(), A), f"{list(kw)}: {W.first_difference(out[0].cpu(), A)}"
