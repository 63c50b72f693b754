"""Match along a path: a continuity weight between neighbouring frames (tvc_knn_match_joined_f32, tvc_joined_convert_f32,
tvc_joined_convert_ragged_f32; Engine.knn_match_joined, Generator.convert(continuity=), BatchedStreamInfer(continuity=)).

Contract (include/tinyvc_hip.h): the neighbour a column's weights form around is the anchor of a Viterbi path over the utterance - a state
gains its similarity s_t[e] and c times its affinity a_t[d][e], the cosine of its row to the row chosen for the frame before.
tests/helpers_match_join.py restates it in numpy; anchor_out equals it bit for bit when it is evaluated from the call's OWN sims_out and
affinity_out, `out` equals the anchored mean of the blob's rows bit for bit, and affinity_out itself is held against the fp64 cosine within
770 * 2^-24, the bound sims_out is held to (derived, not measured: the dot carries 18 roundings, each inv a 768-term sum of squares; the
measured maximum over these shapes goes to profiles/match_join_edges.txt)."""
import os

import numpy as np
import pytest
import torch

import helpers_match_join as mj
import helpers_match_weight as mw
import helpers_workspace as W
from helpers import state_dicts
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
INF = float("inf")
AFF_TOL = 770 * 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = {}


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


def _index(n, seed, half=False):
    """planted_index's rows as an index tensor [1, 768, n] on the device"""
    rows, _q, _a = mw.planted_index(n, seed=seed)
    t = torch.from_numpy(rows.T.copy())[None]
    return (t.half() if half else t).to(DEV)


@pytest.fixture(scope="module")
def targets():
    """four indices of 300 to 600 rows on planted_index: fp32, fp32, fp16 storage, fp32 - every search is the exact kernel's"""
    return [_index(300, 21), _index(450, 22), _index(600, 23, half=True), _index(512, 24)]


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _rows(t):
    """an index tensor [1, 768, N] (fp32 or fp16) -> the rows the gather reads, [N, 768] fp32 on the host"""
    return t[0].float().t().contiguous().cpu().numpy()


def _inv(blob, t):
    """inv [N] as the prepared blob of index tensor t holds it (knn_blob.h: behind the header in an fp16 blob, behind the rows and the bf16x3
    image in an fp32 one)"""
    n = t.shape[2]
    npad = (n + 127) // 128 * 128
    at = 64 if t.dtype == torch.float16 else 64 + n * 768 + npad * 768 * 3 // 2
    return blob[at:at + n].cpu().numpy()


def _ints(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _floats(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def near_source(terms, T, seed=11):
    """test_gpu_match_weight.py's: queries whose four nearest rows lie close together (cosine gaps of 0 to a few hundredths, no ties), so
    that the widths reach the inside of the ramp and a join of a few hundredths decides: terms[b] = the index tensors row b searches"""
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
    "shared": ([[2], [2], [2]], None),                                       # one fp16-kind blob in every row: one segment of the search
    "table": ([[0], [1], [3]], None),                                        # a blob, and a segment, per row
    "blend": ([[0, 1], [1, 2], [2, 3]], [[0.7, 0.3], [1.2, -0.2], [0.5, 0.5]]),      # M = 2, a negative weight too: every term a path of its own
}
KS = [[4, 3, 2], [2, 4, 3], [3, 1, 4]]
WIDTHS = [[0.02, 0.005, 0.0], [0.005, 0.0, 0.02], [INF, 0.02, 0.005]]
CS = [[0.5, 0.05, 2.0], [0.0, 1.0, 0.3], [0.3, 0.5, 0.5]]


def _form(targets, form):
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    pos, w = FORMS[form]
    terms = [[targets[p] for p in row] for row in pos]
    blobs, ns = prepare_references([t for row in terms for t in row])
    return terms, blobs, ns, (_floats(w) if w is not None else None)


def restate(src, terms, sims, idx, anchors, k, width, weights=None, share=None):
    """the definition behind the path, from the call's own lists and anchors: src [B, 768, T], terms[b][m] index tensors, sims / idx
    [M, B, T, 4], anchors [M, B, T], k / width one per row, weights [B, M] or None, share [B, T] or None -> out [B, 768, T]"""
    src = src.cpu().numpy()
    sims, idx, anchors = sims.cpu().numpy(), idx.cpu().numpy(), anchors.cpu().numpy()
    B, _, T = src.shape
    out = np.zeros_like(src)
    for b in range(B):
        acc = None
        for m, t in enumerate(terms[b]):
            mu = mj.match(sims[m, b], idx[m, b], _rows(t), anchors[m, b], k[b], width[b])      # [T, 768]
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


def restate_anchors(sims, aff, k, c):
    """the path from the call's own sims_out [M, B, T, 4] and affinity_out [M, B, T, 4, 4]; k, c one per row -> [M, B, T] int32"""
    sims, aff = sims.cpu().numpy(), aff.cpu().numpy()
    M, B, T = sims.shape[:3]
    got = mj.paths(sims.reshape(M * B, T, 4), aff.reshape(M * B, T, 4, 4), np.tile(np.asarray(k), M), np.tile(np.asarray(c, F), M))
    return torch.from_numpy(got.reshape(M, B, T))


# ---- 1. the affinities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp32", "fp16"])
def test_affinities_are_the_cosines(targets, kind):
    """affinity_out against the fp64 cosine dot / ((|u| + 1e-6) (|v| + 1e-6)) of the rows idx_out names, as the blob holds them; frame 0's
    are zeros; and bit for bit the stated order (helpers_match_join.dot) with the blob's own inv"""
    eng = _engine()
    t = targets[2] if kind == "fp16" else targets[0]
    terms = [[t]] * 3
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    blobs, ns = prepare_references([t] * 3)
    s = near_source(terms, 45)
    _out, idx, aff = eng.knn_match_joined(s.to(DEV), blobs, ns, _floats([0.5] * 3), want_indices=True, want_affinities=True)
    assert aff.shape == (1, 3, 45, 4, 4) and aff.dtype == torch.float32
    rows = _rows(t)
    r64 = rows.astype(np.float64)
    inv64 = 1.0 / (np.linalg.norm(r64, axis=1) + 1e-6)
    worst = 0.0
    for b in range(3):
        i = idx[0, b].cpu().numpy()
        got = aff[0, b].cpu().numpy()
        assert not got[0].any(), "frame 0 has no frame before it"
        ref = np.einsum("tdc,tec->tde", r64[i[:-1]], r64[i[1:]]) * inv64[i[:-1]][:, :, None] * inv64[i[1:]][:, None, :]
        worst = max(worst, float(np.abs(got[1:].astype(np.float64) - ref).max()))
        want = mj.affinities(rows, _inv(blobs[b], t), i)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{kind} row {b}: the affinities are not the stated order's bits"
    print(f"[match_join] {kind}: max |affinity_out - fp64 cosine| = {worst:.3e} (bound {AFF_TOL:.3e})")
    EDGES[kind] = worst
    try:
        with open(os.path.join(ROOT, "profiles", "match_join_edges.txt"), "w") as f:
            f.write("max |affinity_out - fp64 cosine| over tests/test_gpu_match_join.py::test_affinities_are_the_cosines (bound 770 * 2^-24 = 4.590e-05)\n")
            for name, v in sorted(EDGES.items()):
                f.write(f"{name} {v:.3e}\n")
    except OSError:
        pass
    assert worst <= AFF_TOL, (kind, worst)


# ---- 2. the path's bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 64, 65, 200])
def test_path_bits(targets, T, B):
    """anchor_out equals the restatement run on the kernel's own sims_out and affinity_out; k mixed across the rows, c too.  The lengths
    cover the 32-column tile and the path kernel's 64-frame chunk; 257 equal rows are 65 workgroups of the one uniform launch (equal rows
    take no row table: test_ragged_paths_past_one_row_table covers the 256-row chunks)"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    blobs, ns = prepare_references([targets[b % 4] for b in range(B)])
    src = torch.randn(B, 768, T, generator=torch.Generator().manual_seed(100 * T + B)).to(DEV)
    k = [(b + T) % 4 + 1 for b in range(B)]
    c = [(0.0, 0.3, 0.5, 1.0, 2.0)[(b + T) % 5] for b in range(B)]
    out, idx, sims, anchors, aff = eng.knn_match_joined(src, blobs, ns, _floats(c), _ints(k), _floats([0.01] * B), want_indices=True, want_similarities=True,
                                                        want_anchors=True, want_affinities=True)
    assert anchors.shape == (1, B, T) and anchors.dtype == torch.int32
    want = restate_anchors(sims, aff, k, c)
    assert torch.equal(anchors.cpu(), want), f"T {T} B {B}: {int((anchors.cpu() != want).sum())} anchors differ"
    assert int(anchors.min()) >= 0 and bool((anchors[0].cpu() < torch.tensor(k)[:, None]).all())
    if T >= 31 and B >= 3:
        assert bool((anchors != 0).any()), "the path never left neighbour 0: the comparison shows little"


# ---- 3. the stage's bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["plain", "alpha", "protect"])
@pytest.mark.parametrize("form", list(FORMS))
def test_stage_bits(targets, form, mix):
    """out equals the anchored mean of the blob's rows, from the call's own sims_out, idx_out and anchor_out; the anchors equal the path"""
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    T = 45
    s = near_source(terms, T)
    s_d = s.to(DEV)
    B = 3
    _mu, plain_idx = (eng.knn_match_blend(s_d, blobs, ns, w, want_indices=True) if w is not None else eng.knn_match_multi(s_d, blobs, ns, want_indices=True))
    plain_idx = plain_idx if w is not None else plain_idx[None]
    kw, share = {}, None
    if mix != "plain":
        kw["alpha"] = _floats([0.0, 0.35, 1.5])
        share = np.repeat(np.array([0.0, 0.35, 1.5], F)[:, None], T, axis=1)
    if mix == "protect":
        f0 = torch.full((B, T), 150.0)
        f0[0, :7] = 0.0
        f0[1, 10::3] = 0.0
        f0[2, 20:30] = -1.0
        f0[2, 44] = float("nan")
        kw["f0"], kw["protect"] = f0.to(DEV), _floats([0.5, 1.0, 0.25])
        share = eng.frame_share(kw["f0"], [b * T for b in range(B)], [T] * B, kw["alpha"], kw["protect"]).cpu().numpy()
    moved = 0
    for ks, widths, cs in zip(KS, WIDTHS, CS):
        out, idx, sims, anchors, aff = eng.knn_match_joined(s_d, blobs, ns, _floats(cs), _ints(ks), _floats(widths), weights=w, want_indices=True,
                                                            want_similarities=True, want_anchors=True, want_affinities=True, **kw)
        assert torch.equal(idx, plain_idx), f"{form} {mix}: the indices depend on the path"
        assert torch.equal(anchors.cpu(), restate_anchors(sims, aff, ks, cs)), f"{form} {mix} k {ks} c {cs}: the anchors are not the path's"
        want = restate(s, terms, sims, idx, anchors, ks, widths, FORMS[form][1], share)
        assert W.same_bits(out.cpu(), want), f"{form} {mix} k {ks} widths {widths} c {cs}: {W.first_difference(out.cpu(), want)}"
        moved += int((anchors != 0).sum())
    assert moved > 20, f"{form}: the paths hardly ever leave neighbour 0 ({moved} anchors): the comparison shows little"


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_off_is_off(targets, form):
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    s_d = near_source(terms, 45).to(DEV)
    a, p = _floats([0.0, 0.35, 1.5]), _floats([0.5, 1.0, 0.25])
    f0 = torch.full((3, 45), 150.0)
    f0[:, ::4] = 0.0
    f0 = f0.to(DEV)
    k, width = _ints([4, 3, 2]), _floats([0.02, 0.005, 0.01])
    for name, kw in (("plain", {}), ("alpha", dict(alpha=a)), ("protect", dict(alpha=a, protect=p, f0=f0))):
        want = eng.knn_match_weighted(s_d, blobs, ns, k, width, weights=w, **kw)
        out, anchors = eng.knn_match_joined(s_d, blobs, ns, _floats([0.0] * 3), k, width, weights=w, want_anchors=True, **kw)
        assert not anchors.any() and torch.equal(out, want), f"{form} {name}: c = 0 is not the weighted call"
        wide = eng.knn_match_weighted(s_d, blobs, ns, k, _floats([INF] * 3), weights=w, **kw)
        for cs in ([0.5, 2.0, 0.05], [INF, 0.0, 1.0]):
            out, anchors = eng.knn_match_joined(s_d, blobs, ns, _floats(cs), k, _floats([INF] * 3), weights=w, want_anchors=True, **kw)
            assert torch.equal(out, wide), f"{form} {name} c {cs}: the path shows under an infinite width"
        assert bool((anchors != 0).any())      # ... although the path itself moved
        assert torch.equal(eng.knn_match_joined(s_d, blobs, ns, _floats([0.0] * 3), weights=w, **kw),
                           eng.knn_match_weighted(s_d, blobs, ns, weights=w, **kw)), f"{form} {name}: k, width NULL"
    # join = NULL through the joined entry itself is the weighted call (and anchor_out without join is refused)
    lib_out = torch.empty_like(s_d)
    from tinyvc_amd import _lib
    from tinyvc_amd.engine import _ptr
    index, sized = eng._index_args("joined", blobs, ns, w, 3)
    named = dict(index, ctx=eng.ctx, stream=eng._stream(), src=_ptr(s_d), f0=None, alpha=None, protect=None, neighbours=_ptr(k), width=_ptr(width), join=None,
                 out=_ptr(lib_out), idx_out=None, sims_out=None, anchor_out=None, affinity_out=None, B=3, T=45)
    named["ws"], named["ws_bytes"] = eng._query_ws("tvc_workspace_bytes_match_joined", B=3, L=45 * 480, **sized)
    assert eng.lib.tvc_knn_match_joined_f32(*_lib.arguments("tvc_knn_match_joined_f32", named)) == 0
    assert torch.equal(lib_out, eng.knn_match_weighted(s_d, blobs, ns, k, width, weights=w)), f"{form}: join = NULL is not the weighted call"
    named["anchor_out"] = _ptr(torch.empty(3, 45, dtype=torch.int32, device=DEV))
    assert eng.lib.tvc_knn_match_joined_f32(*_lib.arguments("tvc_knn_match_joined_f32", named)) != 0


# ---- 5. no crossing --------------------------------------------------------------------------------------------------------------------------
def test_a_path_never_crosses_a_row(targets):
    """Row b of a batch has the anchors, the affinities and the output of its own B = 1 call.  The boundary is planted: row b ends on a
    query that is row Y of the index, row b + 1 begins on 2 X + Y - X ahead by 0.45 in cosine, more than the frames behind it can move
    (c = 2 times affinities below 0.16 between unrelated rows) and less than the 2 a path that crossed would gain by entering row b + 1 on Y;
    the restatement run across the boundary confirms that it would differ."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    eng = _engine()
    t = targets[0]
    rows = _rows(t)
    B, T = 3, 33
    blobs, ns = prepare_references([t] * B)
    src = near_source([[t]] * B, T, seed=31).numpy()
    X, Y = 60, 61
    for b in range(B - 1):
        src[b, :, T - 1] = rows[Y]
        x, y = rows[X].astype(np.float64), rows[Y].astype(np.float64)
        src[b + 1, :, 0] = (2 * x + y).astype(F)      # cosines 0.894 and 0.447
    s_d = torch.from_numpy(src).to(DEV)
    k, width, c = [4, 4, 4], [0.01, 0.005, 0.02], [2.0, 2.0, 2.0]
    out, idx, sims, anchors, aff = eng.knn_match_joined(s_d, blobs, ns, _floats(c), _ints(k), _floats(width), want_indices=True, want_similarities=True,
                                                        want_anchors=True, want_affinities=True)
    for b in range(B):
        one = eng.knn_match_joined(s_d[b:b + 1].contiguous(), blobs[b:b + 1], ns[b:b + 1], _floats(c[b:b + 1]), _ints(k[b:b + 1]), _floats(width[b:b + 1]),
                                   want_indices=True, want_similarities=True, want_anchors=True, want_affinities=True)
        for got, want, name in zip((out[b:b + 1], idx[:, b:b + 1], sims[:, b:b + 1], anchors[:, b:b + 1], aff[:, b:b + 1]), one, ("out", "idx", "sims", "anchors", "aff")):
            assert W.same_bits(got.cpu().contiguous(), want.cpu()), f"row {b}: {name} != its own B = 1 call"
    # what a crossing path would have chosen: the three rows as ONE utterance, the boundary frames' affinities from the restatement
    i = idx[0].cpu().numpy().reshape(B * T, 4)
    cross_aff = mj.affinities(rows, _inv(blobs[0], t), i)
    crossing = mj.path(sims[0].cpu().numpy().reshape(B * T, 4), cross_aff, 4, 2.0).reshape(B, T)
    own = anchors[0].cpu().numpy()
    for b in range(1, B):
        assert i.reshape(B, T, 4)[b, 0, 0] == X and i.reshape(B, T, 4)[b, 0, 1] == Y, "the plant does not hold"
        assert crossing[b, 0] == 1 and own[b, 0] != crossing[b, 0], f"row {b}: a crossing path would not differ here ({crossing[b, 0]}, {own[b, 0]})"


# ---- 6. totality -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["table", "blend"])
def test_whatever_the_arrays_hold_gives_anchors_and_features(targets, form):
    eng = _engine()
    terms, blobs, ns, w = _form(targets, form)
    s = near_source(terms, 45)
    s[0, :, 3] = float("nan")
    s[1, 5, 40:] = float("inf")
    s_d = s.to(DEV)
    nan = float("nan")
    for join, width, k in (([nan, -1.0, INF], [0.01, 0.01, 0.01], [4, 4, 4]), ([INF, INF, 3e38], [nan, -1.0, 0.0], [-7, 1000, 3]),
                           ([0.5, -INF, 1e30], [INF, 1e-30, 0.005], [0, 2, 5])):
        out, idx, sims, anchors, aff = eng.knn_match_joined(s_d, blobs, ns, _floats(join), _ints(k), _floats(width), weights=w, want_indices=True,
                                                            want_similarities=True, want_anchors=True, want_affinities=True)
        kk = torch.tensor(k).clamp(1, 4)
        assert int(anchors.min()) >= 0 and bool((anchors.cpu() < kk[None, :, None]).all()), (join, width, k)
        assert torch.equal(anchors.cpu(), restate_anchors(sims, aff, k, join)), (join, width, k)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(aff).all()), (join, width, k)
        for m in range(idx.shape[0]):
            for b in range(3):
                assert int(idx[m, b].max()) < terms[b][m].shape[2]


# ---- 7. the fused conversion -----------------------------------------------------------------------------------------------------------------
B2, T2 = 2, 28
SHIFTS2 = [2.0, -3.0]
K2, WIDTH2, C2 = [4, 3], [0.02, 0.005], [0.5, 1.0]


def _stages(gen, wf):
    from tinyvc_amd.module import utils
    eng = gen.engine()
    w = utils.autopad_waveform(wf.to(DEV))
    ssl, f0, logits = eng.encoder(utils.spectrogram(w), want_logits=True)
    return eng, ssl, f0, logits, utils.estimate_energy(w)


def test_convert_equals_its_stage_composition(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, prepare_references
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    eng, ssl, f0, _logits, energy = _stages(gen, wf)
    tg = [targets[1], targets[2]]
    blobs, ns = prepare_references(tg)
    f0s = eng.pitch_match(f0, pitch_shift=SHIFTS2, want_shifted=True)[3]
    weighted = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2)
    for kw, mkw in ((dict(k=K2, match_width=WIDTH2, continuity=C2), dict(neighbours=_ints(K2), width=_floats(WIDTH2), join=_floats(C2))),
                    (dict(match_width=_floats([0.01, 0.0]), continuity=_floats([2.0, 0.3])), dict(width=_floats([0.01, 0.0]), join=_floats([2.0, 0.3]))),
                    (dict(k=_ints([3, 2]), match_width=0.02, continuity=0.5, alpha=[0.3, 0.0]),
                     dict(neighbours=_ints([3, 2]), width=_floats([0.02] * 2), join=_floats([0.5] * 2), alpha=_floats([0.3, 0.0])))):
        out = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, **kw)
        matched, anchors = eng.knn_match_joined(ssl, blobs, ns, want_anchors=True, **mkw)
        assert torch.equal(out, eng.decoder(matched, f0s, energy, angle)), f"{kw}: convert != the stages, knn_match_joined, the decoder"
        assert bool((anchors != 0).any()), f"{kw}: the path never left neighbour 0"
        for b in range(B2):      # a row equals its own call
            one = {n: (v[b:b + 1].contiguous() if isinstance(v, torch.Tensor) else v[b] if isinstance(v, list) else v) for n, v in kw.items()}
            y = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), **one)
            assert torch.equal(out[b:b + 1], y), f"{kw}: row {b} != its own B = 1 call"
    assert not torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2, continuity=C2), weighted), "the path changed nothing"
    # off is off: continuity 0 is the weighted call; under an infinite width tensor any continuity is the call without it
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2, continuity=0.0), weighted)
    assert torch.equal(gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, match_width=_floats([INF, INF]), continuity=1.0),
                       gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle))
    # one shared index takes the same entry; a blend target: every term a path of its own, row by row its own call
    shared = gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, match_width=0.01)
    assert torch.equal(gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, match_width=0.01, continuity=0.0), shared)
    assert not torch.equal(gen.convert(wf.to(DEV), targets[1], 1.0, noise_angle=angle, match_width=0.01, continuity=[0.0, 1.0]), shared)
    blend = Blend([[targets[0], targets[1]], [targets[2], targets[3]]], torch.tensor([[0.7, 0.3], [0.25, 0.75]], device=DEV))
    ob = gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2, continuity=C2)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), Blend([blend.terms[0][b], blend.terms[1][b]], blend.weights[b].tolist()), SHIFTS2[b],
                          noise_angle=angle[b:b + 1].contiguous(), k=K2[b], match_width=WIDTH2[b], continuity=C2[b])
        assert torch.equal(ob[b:b + 1], one), f"row {b}: the batched joined blend != its B = 1 call"
    assert not torch.equal(ob, gen.convert(wf.to(DEV), blend, SHIFTS2, noise_angle=angle, k=K2, match_width=WIDTH2))


def test_convert_with_every_other_keyword(gen, targets):
    """tune, the pitch path, protect and auto_pitch beside the path: continuity 0 is the call without it, the joined call differs from it and
    every row equals its own B = 1 call"""
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41), synth.synth_angle(B2, T2, 42).to(DEV)
    tg = [targets[1], targets[2]]
    reg = torch.tensor([180.0, 240.0], device=DEV)
    kw = dict(tune="chromatic", f0_estimation="viterbi", protect=[0.5, 1.0], k=K2, match_width=WIDTH2)
    plain, sh0 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, **kw)
    same, sh1 = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, continuity=0.0, **kw)
    assert torch.equal(same, plain) and torch.equal(sh1, sh0)
    out, sh = gen.convert(wf.to(DEV), tg, SHIFTS2, noise_angle=angle, auto_pitch=reg, return_shift=True, continuity=C2, **kw)
    assert torch.equal(sh, sh0), "the shifts found on the device depend on the path"
    assert torch.isfinite(out).all() and not torch.equal(out, plain)
    for b in range(B2):
        one = gen.convert(wf[b:b + 1].to(DEV), tg[b], SHIFTS2[b], noise_angle=angle[b:b + 1].contiguous(), auto_pitch=reg[b:b + 1].contiguous(), k=K2[b],
                          match_width=WIDTH2[b], continuity=C2[b], tune="chromatic", f0_estimation="viterbi", protect=kw["protect"][b])
        assert torch.equal(out[b:b + 1], one), f"row {b} != its own B = 1 call"


def test_convert_ragged(gen, targets):
    """a ragged pair, 28 and 21 frames: each utterance equals the stage composition over its own length and its own B = 1 call, which holds
    its start, its length and its row in the batch's tables (the boundary is not planted here: a path cannot cross because frame 0 of an
    utterance reads no affinity, which test_a_path_never_crosses_a_row shows on planted rows)"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_references
    frames = [28, 21]
    lens = [f * 480 for f in frames]
    wf = synth.synth_wave(2, 28 * 480, seed=51)
    wf[1, lens[1]:] = 0
    angle = synth.synth_angle(2, 28, 61).to(DEV)
    for tg in ([targets[1], targets[0]], [targets[2], targets[2]]):      # a blob per utterance; one blob, one segment across the boundary
        out = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, k=K2, match_width=_floats(WIDTH2), continuity=C2)
        weighted = gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, k=K2, match_width=_floats(WIDTH2))
        assert torch.equal(gen.convert(wf.to(DEV), tg, -2.0, noise_angle=angle, lengths=lens, k=K2, match_width=_floats(WIDTH2), continuity=0.0), weighted)
        assert not torch.equal(out, weighted)
        blobs, ns = prepare_references(tg)
        for b, f in enumerate(frames):
            eng, ssl, f0, _logits, energy = _stages(gen, wf[b:b + 1, :lens[b]])
            matched = eng.knn_match_joined(ssl, blobs[b:b + 1], ns[b:b + 1], _floats(C2[b:b + 1]), _ints(K2[b:b + 1]), _floats(WIDTH2[b:b + 1]))
            want = eng.decoder(matched, eng.shift_frequency(f0, -2.0), energy, angle[b:b + 1, :, :f].contiguous())
            assert torch.equal(out[b:b + 1, :lens[b]], want), f"utterance {b} of {f} frames != its own stage composition"
            assert not out[b, lens[b]:].any()
            one = gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tg[b], -2.0, noise_angle=angle[b:b + 1, :, :f].contiguous(), k=K2[b], match_width=WIDTH2[b],
                              continuity=C2[b])
            assert torch.equal(out[b:b + 1, :lens[b]], one), f"utterance {b} != its own B = 1 call"


@pytest.mark.parametrize("form", ["table", "blend"])
def test_ragged_paths_past_one_row_table(gen, targets, form):
    """A ragged batch's (term, utterance) paths travel by value, 256 to a launch: 260 utterances of 12 .. 20 frames (one length class), and
    130 utterances against a two-term Blend (260 paths: term 1's start at term * columns + the utterance's), k, width and c mixed.
    Utterances on both sides of path 256 equal their own B = 1 call bit for bit, and the batch differs from the weighted call."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend
    U = 260 if form == "table" else 130
    rng = np.random.default_rng(97)
    frames = [int(f) for f in rng.integers(12, 21, U)]
    lens = [f * 480 for f in frames]
    wf = synth.synth_wave(U, 20 * 480, seed=71)
    for u in range(U):
        wf[u, lens[u]:] = 0
    angle = synth.synth_angle(U, 20, 72).to(DEV)
    ks = [u % 3 + 2 for u in range(U)]
    widths = [(0.02, 0.005, 0.0, 0.01)[u % 4] for u in range(U)]
    cs = [(0.5, 2.0, 0.0, 1.0, 0.3)[u % 5] for u in range(U)]
    shifts = [float(u % 7 - 3) for u in range(U)]
    if form == "table":
        tg = [targets[u % 4] for u in range(U)]
        one_target = lambda u: tg[u]
        held = [0, 1, 254, 255, 256, 257, 259]
    else:
        w = torch.tensor([[0.7, 0.3], [0.25, 0.75], [1.2, -0.2]], device=DEV)[torch.arange(U) % 3].contiguous()
        tg = Blend([[targets[u % 4] for u in range(U)], [targets[(u + 1) % 4] for u in range(U)]], w)
        one_target = lambda u: Blend([tg.terms[0][u], tg.terms[1][u]], w[u].tolist())
        held = [0, 125, 126, 127, 129]      # term 1 of utterance 126 is path 256
    out = gen.convert(wf.to(DEV), tg, shifts, noise_angle=angle, lengths=lens, k=ks, match_width=widths, continuity=cs)
    weighted = gen.convert(wf.to(DEV), tg, shifts, noise_angle=angle, lengths=lens, k=ks, match_width=widths)
    differ = [u for u in range(U) if not torch.equal(out[u], weighted[u])]
    assert len(differ) > U // 4 and any(u >= 128 for u in differ), f"{form}: the path changed {len(differ)} of {U} utterances"
    assert all(cs[u] != 0.0 for u in differ), "an utterance of continuity 0 is its weighted call"
    for u in held:
        f = frames[u]
        one = gen.convert(wf[u:u + 1, :lens[u]].to(DEV), one_target(u), shifts[u], noise_angle=angle[u:u + 1, :, :f].contiguous(), k=ks[u], match_width=widths[u],
                          continuity=cs[u])
        assert torch.equal(out[u:u + 1, :lens[u]], one), f"{form}: utterance {u} of {f} frames != its own B = 1 call"
        assert not out[u, lens[u]:].any()


# ---- 8. streams ------------------------------------------------------------------------------------------------------------------------------
def test_streams_follow_live_continuity_without_a_new_capture(gen, targets):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    S, nblk = 2, 6
    tg = [targets[0], targets[3]]
    blocks = synth.synth_wave(S, nblk * 1920, seed=84).view(S, nblk, 1920).to(DEV)

    def make(use_graph, c=(0.5, 1.0)):
        st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840,
                                use_graph=use_graph, match_width=[0.01, 0.005], continuity=list(c))
        st.init_buffer()
        assert st.continuity.shape == (S,) and st.continuity.dtype == torch.float32
        return st

    sts = {True: make(True), False: make(False)}
    other = make(False, c=(0.5, 0.0))      # stream 1 differs: stream 0 must not notice

    def block(i):
        angle = synth.synth_angle(S, sts[True].input_size // 480, 850 + i).to(DEV)
        return [st.audio_callback(blocks[:, i], noise_angle=angle).clone() for st in (sts[True], sts[False], other)]

    for i in range(3):
        a, b, c = block(i)
        assert torch.equal(a, b), f"block {i + 1}: graph != eager"
        assert torch.equal(a[0], c[0]), f"block {i + 1}: stream 0 depends on stream 1's continuity"
        assert not torch.equal(a[1], c[1]), f"block {i + 1}: stream 1's continuity changed nothing"
    graph3 = sts[True]._graph[1][True][0]                        # captured at block 3
    for st in (sts[True], sts[False], other):                    # the knob moves: in place, on the device
        st.continuity.fill_(0.0)
    still = make(False)                                          # the same stream left at its first values
    for i in range(3):
        still.audio_callback(blocks[:, i], noise_angle=synth.synth_angle(S, still.input_size // 480, 850 + i).to(DEV))
    for i in range(3, nblk):
        a, b, c = block(i)
        assert torch.equal(a, b), f"block {i + 1}: the replay did not follow the new continuity"
        assert sts[True]._graph[1][True][0] is graph3, "changing continuity in place must not capture again"
        y = still.audio_callback(blocks[:, i], noise_angle=synth.synth_angle(S, still.input_size // 480, 850 + i).to(DEV))
        assert not torch.equal(a, y), f"block {i + 1}: fill_ between replays took no effect"
    st = BatchedStreamInfer(gen, n_streams=S, target=tg, pitch_shift=[0.0, 3.0], device=torch.device(DEV), block_size=1920, extra_size=3840)
    st.init_buffer()
    assert st.continuity is None


# ---- 9. the workspace ------------------------------------------------------------------------------------------------------------------------
def _poisoned(name, eng, call):
    """tests/helpers_workspace.py's scheme: the call in a guarded workspace of exactly its queried peak under every fill word equals the call as it is"""
    want = call()
    torch.cuda.synchronize()
    for word, phase in zip(W.FILLS, W.PHASES):
        with W.guarded_workspace(eng, word, phase) as g:
            got = call()
        W.assert_same_bits(got, want, f"{name} under fill {word:#010x} at phase {phase}")
    print(f"[match_join] {name}: carved peak {'+'.join(str(p) for p in g.peaks)} bytes, {len(W.FILLS)} fills passed")


def test_the_joined_entries_in_a_poisoned_workspace_of_their_queried_peak(gen, targets):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath, PitchSnap, prepare_references
    eng = gen.engine()
    wf, angle = synth.synth_wave(B2, T2 * 480, seed=41).to(DEV), synth.synth_angle(B2, T2, 42).to(DEV)
    blobs, ns = prepare_references([targets[1], targets[2]])
    k, width, c, a, p = _ints(K2), _floats(WIDTH2), _floats(C2), _floats([0.25, 0.6]), _floats([0.5, 1.0])
    reg = _floats([150.0, 220.0])

    def tune():
        return PitchSnap(scale="chromatic", low=12, retune_ms=40.0, strength=[1.0, 0.5])

    _poisoned("joined convert", eng, lambda: eng._convert("joined", wf, blobs, ns, SHIFTS2, angle, None, None, reg, alpha=a, protect=p, path=PitchPath(),
                                                           tune=tune(), neighbours=k, width=width, join=c))
    lens = [28 * 480, 21 * 480]
    rag = wf.clone()
    rag[1, lens[1]:] = 0
    _poisoned("joined convert_ragged", eng, lambda: eng._convert("joined", rag, blobs, ns, SHIFTS2, angle, lens, None, reg, alpha=a, protect=p, path=PitchPath(),
                                                                  tune=tune(), neighbours=k, width=width, join=c))
    s_d = near_source([[targets[1]], [targets[2]]], 45).to(DEV)
    f0 = torch.full((2, 45), 150.0)
    f0[:, ::4] = 0.0
    f0 = f0.to(DEV)
    _poisoned("knn_match_joined", eng, lambda: eng.knn_match_joined(s_d, blobs, ns, c, k, width, alpha=a, f0=f0, protect=p, want_indices=True,
                                                                    want_similarities=True, want_anchors=True, want_affinities=True))
    w = _floats([[0.7, 0.3]])
    bl, bn = prepare_references([targets[0], targets[3]])
    _poisoned("knn_match_joined blend", eng, lambda: eng.knn_match_joined(s_d[:1].contiguous(), bl, bn, c[:1].contiguous(), k[:1].contiguous(),
                                                                          width[:1].contiguous(), weights=w, want_anchors=True))


# ---- 10. the point ---------------------------------------------------------------------------------------------------------------------------
def test_the_point_along_a_path_the_anchor_stays_in_the_chain():
    """test_match_join_host.py's planted case through tvc_knn_match_joined_f32: frame by frame the nearest row alternates between the chain A
    and the strangers B; at c = 0 the anchor's row changes set on every frame, at the c chosen on the CPU from the planted margins it stays
    in A on every frame - the flip counts of the CPU restatement"""
    from test_match_join_host import _planted, chosen_c
    eng = _engine()
    flips0, flips_c, c, _idx, chain, strangers = _planted(chosen_c)
    rows, queries, _chain, _strangers, _margin = mj.planted_chain()
    frames = len(chain)
    blob, n = eng.knn_prepare(torch.from_numpy(rows.T.copy())[None].to(DEV))
    s_d = torch.from_numpy(queries.T.copy())[None].to(DEV)      # [1, 768, frames]
    in_a = set(int(r) for r in chain)
    got = []
    for cc in (0.0, c):
        out, idx, anchors = eng.knn_match_joined(s_d, [blob], [n], _floats([cc]), None, _floats([0.0]), want_indices=True, want_anchors=True)
        i, p = idx[0, 0].cpu().numpy(), anchors[0, 0].cpu().numpy()
        picked = i[np.arange(frames), p]
        got.append(mj.flips(picked, in_a))
        # width 0: unit selection - every frame leaves as the path's row's own bits
        assert W.same_bits(out[0].cpu(), torch.from_numpy(rows[picked].T.copy())), f"c = {cc}: {W.first_difference(out[0].cpu(), torch.from_numpy(rows[picked].T.copy()))}"
    assert got == [flips0, flips_c] == [frames - 1, 0], (got, flips0, flips_c)
