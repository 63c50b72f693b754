"""Compacting a speaker index on the device: k-means over a prepared blob (tvc_index_assign_f32 / _update_f32 / _compact_f32,
feature_retrieval.compact_index, extract_index.py --compact).

The reference makes an index smaller by truncating a random permutation (extract_index.py:43-58) and has nothing to compare centroids
with, so the contracts are the project's own: the assignment IS the existing search (column 0 of knn_topk, bit for bit) and agrees with an
fp64 arg-max wherever fp64 can decide; the update is an fp64 mean rounded once, reproducible bit for bit; the fused call equals the loop
of stage calls.  Inputs are planted mixtures generated here (ROWS)."""
import ctypes

import numpy as np
import pytest
import torch

from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# id: (N, K, Kt, sig, seed)
ROWS = {
    "a": (1037, 4, 12, 0.5, 3),         # smallest K; N is no multiple of 64 / 128 / 256; points keep moving for three iterations
    "b": (1037, 37, 12, 0.5, 1),        # odd K; single-member clusters
    "c": (1037, 130, 12, 0.5, 2),       # K crosses a 128-vector image tile
    "d": (8237, 4100, 12, 0.5, 5),      # K >= KNN_COARSE_MIN (4096): the two-stage search; thousands of singleton clusters
    "e": (3000, 37, 3000, 0.0, 7),      # unstructured data: several iterations of movement
    "f": (33068, 37, 12, 0.5, 4),       # more than one default chunk (32 768 + 300); clusters of thousands of members
}
GAP = 1e-5                              # the project's decidability threshold of an fp64 arg-max (test_gpu_cfg3.py, test_gpu_parity.py)
_cache = {}


def planted(row):
    """(X [N, 768] float32 numpy, init [K] int64 numpy) of a row of ROWS."""
    if row not in _cache:
        N, K, Kt, sig, seed = ROWS[row]
        g = np.random.default_rng(seed)
        cen = g.standard_normal((Kt, 768))
        lab = g.integers(0, Kt, N)
        X = (cen[lab] + sig * g.standard_normal((N, 768))).astype(np.float32)
        init = g.permutation(N)[:K]
        _cache[row] = (X, init.astype(np.int64))
    return _cache[row]


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def on_device(eng, row):
    """(points [768, N] on the device, their fp32-kind blob, N, init [K] on the device)"""
    key = ("dev", row)
    if key not in _cache:
        X, init = planted(row)
        pts = torch.from_numpy(X).t().contiguous().to(DEV)
        blob, n = eng.knn_prepare(pts)
        _cache[key] = (pts, blob, n, torch.from_numpy(init).to(DEV))
    return _cache[key]


def sims64(X, cent):
    """fp64 cosine similarities [N, K] of the rows of X (numpy [N, 768]) to the columns of cent (torch [768, K]), with the match's 1e-6."""
    x = torch.from_numpy(X).double()
    c = cent.detach().cpu().double()
    x = x / (x.norm(dim=1, keepdim=True) + 1e-6)
    c = c / (c.norm(dim=0, keepdim=True) + 1e-6)
    return x @ c


# ---- 1. assign equals the existing search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["a", "b", "c", "d"])
def test_assign_is_column_0_of_the_existing_search(eng, row):
    pts, pblob, N, init = on_device(eng, row)
    K = init.numel()
    cblob, _ = eng.knn_prepare(pts[:, init].contiguous())
    sims, idx = eng.knn_topk(pts[None], cblob, K)
    assign, sim, moved = eng.index_assign(pblob, N, cblob, K)
    assert assign.dtype == torch.int64 and assign.shape == (N,) and sim.shape == (N,)
    assert torch.equal(assign, idx[0, :, 0]) and torch.equal(sim, sims[0, :, 0])
    assert int(moved) == N, "assign starts at -1: every entry changes"
    again, _s, moved2 = eng.index_assign(pblob, N, cblob, K, assign=assign)
    assert int(moved2) == 0 and torch.equal(again, idx[0, :, 0])


@pytest.mark.parametrize("row,chunk", [("a", 512), ("f", 0)])      # chunks of 512, 512 and 13; the default chunk: 32 768 and 300
def test_assign_does_not_depend_on_the_chunk(eng, row, chunk):
    pts, pblob, N, init = on_device(eng, row)
    K = init.numel()
    cblob, _ = eng.knn_prepare(pts[:, init].contiguous())
    eng.set_index_assign_chunk(65536)                                # one chunk
    try:
        one, one_s, _m = eng.index_assign(pblob, N, cblob, K)
        eng.set_index_assign_chunk(chunk)
        got, got_s, moved = eng.index_assign(pblob, N, cblob, K)
    finally:
        eng.set_index_assign_chunk(0)
    assert torch.equal(got, one) and torch.equal(got_s, one_s) and int(moved) == N
    sims, idx = eng.knn_topk(pts[None], cblob, K)
    assert torch.equal(got, idx[0, :, 0]) and torch.equal(got_s, sims[0, :, 0])


# ---- 2. assign against fp64, teacher-forced -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(ROWS))
def test_assign_against_an_fp64_arg_max(eng, row):
    """Four iterations on the device; in each the device's own centroids go to the fp64 restatement (so one near-tie cannot derail the
    later iterations).  An iteration in which no point moved leaves the centroids as they were (asserted) and is not restated again."""
    X, _init = planted(row)
    pts, pblob, N, init = on_device(eng, row)
    K = init.numel()
    cent = pts[:, init].contiguous()
    assign = None
    for it in range(4):
        cblob, _ = eng.knn_prepare(cent)
        assign, _sim, moved = eng.index_assign(pblob, N, cblob, K, assign=assign)
        if it and int(moved) == 0:
            before = cent.clone()
            cent, _c = eng.index_update(pblob, N, assign, cent)
            assert torch.equal(cent, before)
            break
        s = sims64(X, cent)
        top = torch.topk(s, 2, dim=1)
        dec = (top.values[:, 0] - top.values[:, 1]) > GAP
        left_out = 1.0 - float(dec.double().mean())
        a = assign.cpu()
        chosen = s.gather(1, a[:, None])[:, 0]
        worst = float((top.values[:, 0] - chosen).max())
        print(f"[index compact] row {row} iteration {it}: moved {int(moved)}, {left_out:.3%} of the points undecidable at {GAP}, worst fp64 shortfall {worst:.2e}")
        assert left_out <= 0.02, f"precondition: row {row} iteration {it}: {left_out:.3%} of the points have an fp64 gap below {GAP}"
        assert torch.equal(a[dec], top.indices[:, 0][dec])
        assert worst <= GAP
        cent, _counts = eng.index_update(pblob, N, assign, cent)


# ---- 3. the update alone --------------------------------------------------------------------------------------------------------------
def update_case(eng, N, K, assign, half, seed):
    g = np.random.default_rng(seed)
    X = g.standard_normal((N, 768)).astype(np.float32)
    X[::5] *= 30.0
    pts = torch.from_numpy(X).t().contiguous().to(DEV)
    if half:
        pts = pts.half()
    held = pts.float().t().cpu().double().numpy()                    # the values the blob holds
    blob, n = eng.knn_prepare(pts)
    cent0 = torch.from_numpy(g.standard_normal((768, K)).astype(np.float32)).to(DEV)
    a = torch.from_numpy(assign).to(DEV)
    cent, counts = eng.index_update(blob, n, a, cent0.clone())
    cent2, counts2 = eng.index_update(blob, n, a, cent0.clone())
    assert torch.equal(cent, cent2) and torch.equal(counts, counts2), "the update is not reproducible bit for bit"
    valid = (assign >= 0) & (assign < K)
    want_counts = np.bincount(assign[valid], minlength=K)
    assert counts.dtype == torch.int32 and counts.cpu().tolist() == want_counts.tolist()
    got = cent.cpu().double().numpy()
    worst = 0.0
    for k in range(K):
        members = np.nonzero(assign == k)[0]
        if members.size == 0:
            assert torch.equal(cent[:, k], cent0[:, k]), f"empty cluster {k} did not keep its centroid"
            continue
        rows = held[members]
        if members.size == 1:
            assert torch.equal(cent[:, k], pts[:, members[0]].float()), f"one-member cluster {k} is not its point"
            continue
        ref = rows.mean(axis=0)
        bound = 2.0 ** -24 * np.abs(ref) + members.size * 2.0 ** -52 * np.abs(rows).mean(axis=0)      # one fp32 rounding + an fp64 sum of n terms
        err = np.abs(got[:, k] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"cluster {k} ({members.size} members): error {err.max():.3e} beyond the rounding bound"
    return worst


@pytest.mark.parametrize("half", [False, True])
def test_update_hand_made_assignments(eng, half):
    N, K = 1037, 37
    g = np.random.default_rng(21)
    assign = g.integers(3, K, N).astype(np.int64)                    # cluster 0 stays empty
    order = g.permutation(N)
    assign[order[:700]] = 2                                          # 700 members scattered over the index range
    assign[order[700]] = 1                                           # one member
    assign[order[701:704]] = -1                                      # no cluster
    assign[order[704]] = K                                           # out of range: must not index memory
    worst = update_case(eng, N, K, assign, half, seed=22)
    print(f"[index compact] update N={N} K={K} {'fp16' if half else 'fp32'} points: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("half", [False, True])
def test_update_one_cluster_of_20000_members(eng, half):
    N, K = 20011, 4
    g = np.random.default_rng(23)
    assign = np.zeros(N, dtype=np.int64)
    assign[g.permutation(N)[:11]] = np.array([1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3])
    worst = update_case(eng, N, K, assign, half, seed=24)
    print(f"[index compact] update N={N}, 20 000 members in one cluster, {'fp16' if half else 'fp32'} points: worst error / bound {worst:.3f}")


# ---- 4. the fused call equals the stage loop ------------------------------------------------------------------------------------------
def stage_loop(eng, pts, pblob, N, init, iters):
    cent = pts[:, init].contiguous()
    assign, hist, cents, moves = None, [], [], []
    for _ in range(iters):
        cblob, K = eng.knn_prepare(cent)
        prev = torch.full((N,), -1, dtype=torch.int64) if assign is None else assign.cpu().clone()
        assign, _s, moved = eng.index_assign(pblob, N, cblob, K, assign=assign)
        assert int(moved) == int((assign.cpu() != prev).sum()), "moved is not the count of changed entries"
        moves.append(int(moved))
        cent, counts = eng.index_update(pblob, N, assign, cent.clone())
        cents.append(cent.clone())
        hist.append(assign.clone())
    blob, _ = eng.knn_prepare(cent)
    return cent, blob, assign, counts, moves, cents


@pytest.mark.parametrize("row,chunk", [("a", 0), ("c", 0), ("e", 0), ("a", 512)])
def test_fused_call_equals_the_stage_loop(eng, row, chunk):
    pts, pblob, N, init = on_device(eng, row)
    cent, blob, assign, counts, moves, cents = stage_loop(eng, pts, pblob, N, init, 4)
    eng.set_index_assign_chunk(chunk)
    try:
        f_index, f_blob, f_assign, f_counts, f_moved = eng.index_compact(pblob, N, init, 4)
    finally:
        eng.set_index_assign_chunk(0)
    print(f"[index compact] row {row} chunk {chunk or 32768}: moved {f_moved.tolist()}")
    assert f_index.shape == (1, 768, init.numel())
    assert torch.equal(f_index[0], cent)
    assert torch.equal(f_blob.view(torch.int32), blob.view(torch.int32))
    assert torch.equal(f_assign, assign) and torch.equal(f_counts, counts)
    assert f_moved.tolist() == moves and moves[0] == N
    assert int(f_counts.sum()) == N
    for i in range(1, 4):
        if moves[i] == 0:
            assert torch.equal(cents[i], cents[i - 1]), f"no point moved in iteration {i}, yet the centroids changed"


def test_compact_arguments_are_validated(eng):
    pts, pblob, N, init = on_device(eng, "a")
    lib, st = eng.lib, eng._stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cent = torch.zeros(768, 4, device=DEV)
    blob = torch.zeros(lib.tvc_knn_prepared_elems(4), device=DEV)
    a = torch.zeros(N, dtype=torch.int64, device=DEV)
    need = ctypes.c_size_t()
    assert lib.tvc_workspace_bytes_index_compact(eng.ctx, N, 3, ctypes.byref(need)) == -1          # K < 4
    assert lib.tvc_workspace_bytes_index_compact(eng.ctx, N, N + 1, ctypes.byref(need)) == -1      # K > N
    assert lib.tvc_workspace_bytes_index_compact(eng.ctx, 1 << 22, (1 << 20) + 1, ctypes.byref(need)) == -1      # above the header's limit
    assert lib.tvc_workspace_bytes_index_compact(eng.ctx, 1 << 22, 131072, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.tvc_index_compact_f32(eng.ctx, st, p(pblob), N, p(init), 4, 0, p(cent), p(blob), None, None, None, None, 0) == -1      # iters < 1
    assert lib.tvc_index_compact_f32(eng.ctx, st, p(pblob), N, p(init), 4, 1, p(cent), p(blob), None, None, None, None, 0) == -4      # no workspace
    assert lib.tvc_index_compact_f32(eng.ctx, st, p(pblob), N + 1, p(init), 4, 1, p(cent), p(blob), None, None, None, None, 0) == -1  # not the blob's N
    assert lib.tvc_index_update_f32(eng.ctx, st, p(pblob), N, None, 4, p(cent), None, None, 0) == -1
    assert lib.tvc_index_assign_f32(eng.ctx, st, p(pblob), N, None, 4, p(a), None, None, None, 0) == -1
    assert lib.tvc_ctx_set_index_assign_chunk(eng.ctx, -1) == -1
    with pytest.raises(ValueError):
        eng.index_compact(pblob, N, init[:3], 2)


# ---- 5. compact_index -------------------------------------------------------------------------------------------------------------------
def test_compact_index(eng):
    from tinyvc_amd.module.tinyvc import compact_index, match_features
    X, init = planted("b")
    pts, _pblob, N, _i = on_device(eng, "b")
    K = init.size
    ref = pts[None].clone()
    src = torch.randn(1, 768, 50, generator=torch.Generator().manual_seed(9)).to(DEV)
    out, info = compact_index(ref, K, iters=3, init_cols=init, return_info=True)
    assert out.shape == (1, 768, K) and out.dtype == torch.float32 and getattr(out, "_tvc_prepared", None) is not None
    assert info["moved"].tolist()[0] == N and int(info["counts"].sum()) == N and info["assign"].shape == (N,)
    assert torch.equal(match_features(src, out), match_features(src, out.clone())), "the blob riding on the result is not the blob of its centroids"
    seeded = compact_index(ref, K, iters=3, generator=torch.Generator().manual_seed(5))
    want_init = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:K]
    assert torch.equal(seeded, compact_index(ref, K, iters=3, init_cols=want_init))
    # an fp16 reference: the points are the fp16 values
    out16 = compact_index(ref.half(), K, iters=3, init_cols=init)
    assert out16.shape == (1, 768, K) and out16.dtype == torch.float32 and torch.isfinite(out16).all()
    # snap: real frames of the speaker
    snapped = compact_index(ref, K, iters=3, init_cols=init, snap=True)
    assert snapped.shape == (1, 768, K) and getattr(snapped, "_tvc_prepared", None) is not None
    assert torch.equal(match_features(src, snapped), match_features(src, snapped.clone()))
    s = sims64(X, out[0]).t()                                          # [K, N]: every centroid against every point
    top = torch.topk(s, 2, dim=1)
    dec = (top.values[:, 0] - top.values[:, 1]) > GAP
    # The fp64 restatement of this row on the CPU (three rounds, then every centroid against every point) has one centroid, number 14 with
    # 34 members, whose two nearest members lie 9.8e-6 apart; the next smallest gap is 4.0e-5.  K = 37 columns are too few for a 2 % rule
    # (it would allow none), so the precondition is a count: at most 2 columns left out.  Every column, decidable or not, must still be
    # within GAP of the best member in fp64.
    print(f"[index compact] snap: {int((~dec).sum())} of {K} columns undecidable at {GAP}: {(~dec).nonzero().flatten().tolist()}")
    assert int((~dec).sum()) <= 2, "precondition: the nearest member of a centroid is decidable in fp64 for all but two columns"
    sn = snapped[0].cpu()
    pts_c = torch.from_numpy(X).t()
    for k in range(K):
        hits = (pts_c == sn[:, k:k + 1]).all(dim=0).nonzero().flatten().tolist()
        assert hits, f"snapped column {k} is no column of the input"
        if dec[k]:
            assert int(top.indices[k, 0]) in hits, f"snapped column {k} is not the fp64-nearest member"
        assert float(top.values[k, 0] - s[k, hits].max()) <= GAP, f"snapped column {k} is further than {GAP} from the fp64-nearest member"
    with pytest.raises(ValueError):
        compact_index(ref, N + 1)
    with pytest.raises(ValueError):
        compact_index(ref, 3)


# ---- 6. extract_index.py --compact --------------------------------------------------------------------------------------------------------
def test_extract_index_compact(tmp_path):
    import extract_index
    from tinyvc_amd.module.tinyvc import compact_index
    d = tmp_path / "clips"
    d.mkdir()
    torch.save(synth.synth_state_dict("encoder"), tmp_path / "encoder.pt")
    for i in range(8):
        audio_io.save(str(d / f"{i}.wav"), synth.synth_wave(1, 9600 + 960 * i - 7 * (i % 2), seed=60 + i), 24000)
    common = ["--dataset-cache", str(d), "-encp", str(tmp_path / "encoder.pt"), "-size", "40", "-d", DEV, "--seed", "3"]
    assert extract_index.main(common + ["-o", str(tmp_path / "plain.pt")]) == 0
    plain = torch.load(tmp_path / "plain.pt")
    assert plain.shape == (1, 768, 40) and plain.dtype == torch.float32
    states = []
    orig = extract_index.compact_index

    def spy(reference, size, **kw):
        states.append(kw["generator"].get_state().clone())
        return orig(reference, size, **kw)

    extract_index.compact_index = spy
    try:
        assert extract_index.main(common + ["-o", str(tmp_path / "compact.pt"), "--compact", "16"]) == 0
    finally:
        extract_index.compact_index = orig
    got = torch.load(tmp_path / "compact.pt")
    assert got.shape == (1, 768, 16) and got.dtype == torch.float32 and len(states) == 1
    g = torch.Generator()
    g.set_state(states[0])
    want = compact_index(plain.to(DEV), 16, generator=g).cpu()
    assert torch.equal(got, want)
    # the run without --compact writes what it wrote before the flag existed: the reference's recipe on the same generator
    gen = torch.Generator().manual_seed(3)
    order = torch.randperm(8, generator=gen).tolist()
    from tinyvc_amd.module.tinyvc import Encoder
    enc = Encoder()
    enc.load_state_dict(torch.load(tmp_path / "encoder.pt", map_location="cpu"))
    enc = enc.eval().to(DEV)
    feats, total = [], 0
    for i in order:
        z = extract_index.encode_clip(enc, torch.device(DEV), str(d / f"{i}.wav"), 4)
        feats.append(z)
        total += z.shape[2]
        if total > 40:
            break
    assert torch.equal(plain, extract_index.assemble(feats, 40, gen, False))
    assert extract_index.main(common + ["-o", str(tmp_path / "half.pt"), "--compact", "16", "--half", "--compact-snap", "--compact-iters", "2"]) == 0
    half = torch.load(tmp_path / "half.pt")
    assert half.shape == (1, 768, 16) and half.dtype == torch.float16
