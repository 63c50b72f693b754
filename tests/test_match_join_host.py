"""The match along a path (tvc_knn_match_joined_f32, tvc_joined_convert_f32, tvc_joined_convert_ragged_f32; Generator.convert(continuity=))
without a GPU: the definition's consequences on its numpy restatement (tests/helpers_match_join.py), the symbols, the refusals of the Python
layer and the entry scripts' arguments."""
import argparse
import inspect
import itertools

import numpy as np
import pytest
import torch

from tinyvc_amd import _lib

import helpers_match_join as mj
import helpers_match_weight as mw

F = np.float32
NEW = ["tvc_knn_match_joined_f32", "tvc_joined_convert_f32", "tvc_joined_convert_ragged_f32", "tvc_workspace_bytes_joined",
       "tvc_workspace_bytes_ragged_joined", "tvc_workspace_bytes_match_joined"]


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _utterance(rng, n):
    """sorted similarities as the lists hold them and affinities in [-1, 1]"""
    sims = np.sort(rng.uniform(0.2, 0.9, (n, 4)).astype(F), axis=1)[:, ::-1].copy()
    aff = rng.uniform(-1, 1, (n, 4, 4)).astype(F)
    aff[0] = 0
    return sims, aff


def _brute(sims, aff, k, c):
    """every one of the k^len paths, totals in fp64 -> (best path, best total - second-best total)"""
    s, a = sims.astype(np.float64), aff.astype(np.float64)
    totals = []
    for p in itertools.product(range(k), repeat=len(s)):
        tot = s[0, p[0]] + sum(s[t, p[t]] + c * a[t, p[t - 1], p[t]] for t in range(1, len(s)))
        totals.append((tot, p))
    totals.sort(key=lambda x: -x[0])
    gap = totals[0][0] - totals[1][0] if len(totals) > 1 else np.inf
    return np.array(totals[0][1], np.int32), gap


# ---- the dynamic programme -------------------------------------------------------------------------------------------------------------
def test_the_dynamic_programme_equals_a_brute_force_over_all_paths():
    """len <= 6, k <= 4; random inputs are kept only where the best and second-best totals differ by more than 1e-3, so fp32 rounding (a
    few 1e-7 per frame) cannot decide"""
    rng = np.random.default_rng(5)
    kept = 0
    for trial in range(400):
        n, k = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        c = float(rng.choice([0.0, 0.05, 0.3, 1.0, 4.0]))
        sims, aff = _utterance(rng, n)
        want, gap = _brute(sims, aff, k, c)
        if gap <= 1e-3:
            continue
        kept += 1
        assert np.array_equal(mj.path(sims, aff, k, c), want), (trial, n, k, c)
    assert kept >= 150


def test_c_0_is_anchor_0_everywhere_and_the_weighted_rule_by_bits():
    rng = np.random.default_rng(6)
    sims, aff = _utterance(rng, 50)
    sims[:10, 1:] = sims[:10, :1] - rng.uniform(0, 0.01, (10, 3)).astype(F).cumsum(axis=1)      # weights inside (0, 1)
    sims[20:24, 1] = sims[20:24, 0]      # exact ties: the lowest e
    rows = rng.standard_normal((64, 24)).astype(F)
    rows[:, 5] = F(-0.0)
    idx = np.stack([rng.permutation(64)[:4] for _ in range(50)])
    for k, width in ((4, 0.02), (3, 0.005), (2, np.inf), (1, 0.02), (4, 0.0)):
        anchors = mj.path(sims, aff, k, 0.0)
        assert (anchors == 0).all(), (k, width)
        w, W = mj.weights(sims, anchors, k, width)
        w0, W0 = mw.weights(sims, k, width)
        assert np.array_equal(bits(w), bits(w0)) and np.array_equal(bits(W), bits(W0))
        assert np.array_equal(bits(mj.match(sims, idx, rows, anchors, k, width)), bits(mw.match(sims, idx, rows, k, width)))


def test_infinite_width_makes_the_path_irrelevant_and_width_0_is_unit_selection():
    rng = np.random.default_rng(7)
    sims, aff = _utterance(rng, 30)
    rows = rng.standard_normal((64, 24)).astype(F)
    idx = np.stack([rng.permutation(64)[:4] for _ in range(30)])
    anchors = mj.path(sims, aff, 4, 2.0)
    assert (anchors != 0).any()      # the path does leave neighbour 0
    assert np.array_equal(bits(mj.match(sims, idx, rows, anchors, 4, np.inf)), bits(mw.match(sims, idx, rows, 4, np.inf)))
    assert (np.diff(sims, axis=1) < 0).all()      # no ties: width 0 stores the path's row's own bits
    assert np.array_equal(bits(mj.match(sims, idx, rows, anchors, 4, 0.0)), bits(rows[idx[np.arange(30), anchors]]))
    assert (mj.path(sims, aff, 1, 2.0) == 0).all()      # k = 1 has no choice to make
    w, W = mj.weights(sims, anchors, 3, 0.05)
    assert (w >= 0).all() and (w <= 1).all() and (W >= 1).all() and (w[np.arange(30), np.minimum(anchors, 3)] >= 0).all()


def test_the_rule_is_total():
    """non-finite similarities and affinities and a bad c give anchors inside 0 .. k - 1, and finite renormalised scores"""
    rng = np.random.default_rng(8)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e-45, 0.5], F)
    for trial in range(60):
        n, k = int(rng.integers(1, 40)), int(rng.integers(-2, 8))
        sims = rng.choice(odd, (n, 4)).astype(F)
        aff = rng.choice(odd, (n, 4, 4)).astype(F)
        c = rng.choice(np.array([np.nan, -1.0, np.inf, -np.inf, 0.0, 3e38, 1.0], F))
        anchors, D = mj.path(sims, aff, k, c, want_scores=True)
        kk = min(max(k, 1), 4)
        assert anchors.min() >= 0 and anchors.max() <= kk - 1, (trial, k, c)
        assert np.isfinite(D).all() and D[:kk].max() == 0
        w, W = mj.weights(sims, anchors, k, rng.choice(np.array([np.nan, -1.0, np.inf, 0.0, 0.02], F)))
        assert (w >= 0).all() and (w <= 1).all() and (W >= 1).all()
    assert mj.continuity(F(np.inf)) == np.finfo(F).max and mj.continuity(F(np.nan)) == 0 and mj.continuity(F(-2)) == 0


def test_renormalised_scores_pick_the_fp64_path_at_15000_frames():
    """gapped inputs: similarities and affinities on a grid of 1/64, so every total is exact in fp64 and, renormalised, in fp32 - the
    accumulated sum of 15 000 frames (about 2^14) would have lost the 1/64 steps' low bits without the subtraction"""
    rng = np.random.default_rng(9)
    n = 15000
    sims = np.sort(rng.integers(13, 58, (n, 4)), axis=1)[:, ::-1].astype(F) / F(64)
    sims += (np.arange(4)[::-1] * F(1 / 256)).astype(F)      # no ties inside a list
    aff = (rng.integers(-64, 65, (n, 4, 4)) / 64).astype(F)
    c = 0.5
    got = mj.path(sims, aff, 4, c)
    # the same recursion in fp64, without renormalisation
    s, a = sims.astype(np.float64), aff.astype(np.float64)
    D = s[0].copy()
    bp = np.zeros((n, 4), np.int64)
    for t in range(1, n):
        cand = D[:, None] + c * a[t]
        bp[t] = cand.argmax(axis=0)      # the first maximum: the lowest d
        D = s[t] + cand.max(axis=0)
    p = int(D.argmax())
    want = np.zeros(n, np.int32)
    for t in range(n - 1, -1, -1):
        want[t] = p
        p = bp[t, p]
    assert np.array_equal(got, want)
    assert (np.diff(got) != 0).sum() > 1000      # a path that moves: the test is not about a constant


def test_the_dot_has_one_order_and_a_cosines_accuracy():
    rng = np.random.default_rng(10)
    u = rng.standard_normal((5, 768)).astype(F)
    v = rng.standard_normal((5, 768)).astype(F)
    d = mj.dot(u, v)
    exact = (u.astype(np.float64) * v).sum(-1)
    assert d.dtype == F and np.abs(d - exact).max() <= 18 * 2.0 ** -24 * (np.abs(u.astype(np.float64) * v)).sum(-1).max()
    rows = u / np.linalg.norm(u, axis=1, keepdims=True)
    a = mj.affinities(rows, mj.blob_inv(rows), np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 0, 1, 2]]))
    assert (a[0] == 0).all() and abs(a[1, 1, 0] - 1) < 1e-5 and abs(a[2, 3, 0] - 1) < 1e-5      # the same row in neighbouring frames


def _planted(c_of):
    """the planted case through the restatement: (flips at c = 0, flips at the chosen c, c)"""
    rows, queries, chain, strangers, margin = mj.planted_chain()
    r64 = rows.astype(np.float64)
    unit = r64 / np.linalg.norm(r64, axis=1, keepdims=True)
    cos = (queries.astype(np.float64) / np.linalg.norm(queries, axis=1, keepdims=True)) @ unit.T
    idx = np.argsort(-cos, axis=1, kind="stable")[:, :4]
    sims = np.take_along_axis(cos, idx, 1).astype(F)
    aff = mj.affinities(rows, mj.blob_inv(rows), idx)
    c = c_of(rows, chain, strangers, margin)
    in_a = set(int(r) for r in chain)
    out = []
    for cc in (0.0, c):
        anchors = mj.path(sims, aff, 4, cc)
        out.append(mj.flips(idx[np.arange(len(idx)), anchors], in_a))
    return out[0], out[1], c, idx, chain, strangers


def chosen_c(rows, chain, strangers, margin):
    """from the planted margins alone: leaving A for one frame gains at most `margin` in similarity and loses two joins, each worth at least
    (the smallest affinity inside A) - (the largest between A and B) - so twice the margin over that difference settles every frame"""
    unit = rows.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    inside = (unit[chain] @ unit[chain].T)[~np.eye(len(chain), dtype=bool)].min()
    across = np.abs(unit[chain] @ unit[strangers].T).max()
    return float(2 * margin / (inside - across))


def test_the_point_along_a_path_the_anchor_stays_in_the_chain():
    """The point, on the restatement.  A planted index: a chain A of rows mutually close from frame to frame, a set B far from A and from
    each other; the nearest row alternates between A and B by a small margin.  At c = 0 the anchor's row changes set on every frame; at a c
    chosen from the planted margins it stays in A on every frame."""
    flips0, flips_c, c, idx, chain, strangers = _planted(chosen_c)
    frames = len(chain)
    nearest = idx[:, 0]
    assert all(nearest[t] == (strangers[t] if t % 2 == 0 else chain[t]) for t in range(frames))      # the plant holds
    assert flips0 == frames - 1
    assert 0 < c < 0.1 and flips_c == 0


# ---- the C ABI and the Python layer ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _names(decl, name):
    return [a.split()[-1].lstrip("*") for a in decl[name]]


def test_symbols_are_declared_bound_and_exported(lib):
    from test_cabi import header_functions
    decl = header_functions()
    for name in NEW:
        assert name in decl, f"{name} is not declared in tinyvc_hip.h"
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0], f"{name} is not bound with its signature"
    # each fused entry is its weighted sibling's argument list plus join, behind width
    for name, sibling in (("tvc_joined_convert_f32", "tvc_weighted_convert_f32"), ("tvc_joined_convert_ragged_f32", "tvc_weighted_convert_ragged_f32")):
        args, sib = _names(decl, name), _names(decl, sibling)
        at = args.index("join")
        assert args[at - 1] == "width" and args[:at] + args[at + 1:] == sib, name
        assert _lib.SIGNATURES[name][1][:at] + _lib.SIGNATURES[name][1][at + 1:] == _lib.SIGNATURES[sibling][1], name
    # the stage call: the weighted stage call plus join behind width, and anchor_out and affinity_out behind sims_out
    args = _names(decl, "tvc_knn_match_joined_f32")
    assert args[args.index("join") - 1] == "width" and args[args.index("anchor_out") - 1] == "sims_out" and args[args.index("affinity_out") - 1] == "anchor_out"
    assert [a for a in args if a not in ("join", "anchor_out", "affinity_out")] == _names(decl, "tvc_knn_match_weighted_f32")
    # argument checks come before any device work: no context, no call
    assert lib.tvc_knn_match_joined_f32(*([None] * 6), 1, *([None] * 11), 1, 1, None, 0) == -1
    from tinyvc_amd import engine
    assert callable(engine.Engine.knn_match_joined)
    params = inspect.signature(engine.Engine.knn_match_joined).parameters
    assert "want_anchors" in params and "want_affinities" in params
    assert engine._names("joined", False) == ("tvc_workspace_bytes_joined", "tvc_joined_convert_f32")
    assert engine._names("joined", True) == ("tvc_workspace_bytes_ragged_joined", "tvc_joined_convert_ragged_f32")
    assert engine._names("joined") == ("tvc_workspace_bytes_match_joined", "tvc_knn_match_joined_f32")
    assert engine._FEATURES_OFF["join"] is None


def test_continuity_is_normalised_on_the_host():
    from tinyvc_amd.module.tinyvc.feature_retrieval import continuity_rows, resolve_continuity, resolve_match_width
    inf = float("inf")
    assert resolve_continuity(0.5, 2, [0.02, 0.02]) == [0.5, 0.5] and resolve_continuity([0.0, 1.5], 2, [inf, 0.02]) == [0.0, 1.5]
    assert resolve_continuity(0.0, 3) == [0.0] * 3 and resolve_continuity(0, 2, [inf, inf]) == [0.0, 0.0]      # 0 needs no width
    rows = continuity_rows(resolve_continuity([0.5, 2.0], 2, resolve_match_width(0.0, 2)), 2, "cpu")
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.tolist() == [0.5, 2.0]
    for bad, why in ((-0.1, ">= 0"), (float("nan"), ">= 0"), ([0.1, -1.0], ">= 0"), ("0.1", "continuity"), (True, "continuity"),
                     ([0.1] * 3, "3 shares for a batch of 2"), (torch.zeros(2), "lives on the GPU"), (torch.zeros(2, dtype=torch.float64), "fp32")):
        with pytest.raises(ValueError, match=why):
            resolve_continuity(bad, 2, [0.02, 0.02])
    # the infinite-width refusal names both keywords
    for width in (None, [inf, inf]):
        with pytest.raises(ValueError, match="continuity") as e:
            resolve_continuity(0.5, 2, width)
        assert "match_width" in str(e.value)


@pytest.fixture(scope="module")
def cpu_gen():
    """a Generator that never left the CPU: whatever reaches its engine raises TinyVCError (a RuntimeError), never ValueError"""
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_refusals_come_before_device_work(cpu_gen):
    wf = torch.zeros(2, 4800)
    plain = torch.zeros(1, 768, 8)
    for bad in (-0.5, float("nan"), [0.1, 0.2, 0.3], "0.1", torch.zeros(2)):
        with pytest.raises(ValueError, match="continuity"):
            cpu_gen.convert(wf, plain, 0.0, continuity=bad, match_width=0.02)
    for kw in (dict(continuity=0.5), dict(continuity=0.5, match_width=float("inf")), dict(continuity=[0.0, 0.5], k=2)):
        with pytest.raises(ValueError, match="continuity") as e:
            cpu_gen.convert(wf, plain, 0.0, **kw)
        assert "match_width" in str(e.value)
    with pytest.raises(ValueError, match="continuity"):
        cpu_gen.convert(wf, [plain, plain], [0.0, 1.0], continuity=-1.0, match_width=0.02, lengths=[4800, 2400], alpha=0.5)
    # a well-formed call gets as far as the device - and there is none; None never looks at it
    for kw in (dict(continuity=0.5, match_width=0.02), dict(continuity=0.0), dict(continuity=[0.5, 0.0], match_width=[0.02, float("inf")], k=2),
               dict(continuity=None)):
        with pytest.raises(_lib.TinyVCError):
            cpu_gen.convert(wf, plain, 0.0, **kw)
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    with pytest.raises(ValueError, match="continuity"):
        BatchedStreamInfer(cpu_gen, n_streams=2, continuity=-0.01, match_width=0.02, device="cuda")
    with pytest.raises(ValueError, match="match_width"):
        BatchedStreamInfer(cpu_gen, n_streams=2, continuity=0.5, device="cuda")
    with pytest.raises(ValueError, match="continuity"):
        StreamInfer(cpu_gen, continuity=float("nan"), match_width=0.02)
    st = BatchedStreamInfer(cpu_gen, n_streams=2, device="cuda")
    assert st.continuity is None


def test_entry_scripts_parse_continuity_and_leave_the_call_alone_without_it(capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.tinyvc.feature_retrieval import continuity_keywords, match_weight_keywords
    for mod, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        absent = mod.build_parser().parse_args([])
        assert absent.continuity is None
        assert continuity_keywords(absent, name, {}) == {} and capsys.readouterr().out == ""      # nothing added to the call, nothing printed
        given = mod.build_parser().parse_args(["--continuity", "0.5", "--match-width", "0.02"])
        kw = match_weight_keywords(given, name)
        capsys.readouterr()
        assert continuity_keywords(given, name, kw) == {"continuity": 0.5}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "0.5" in out
        assert continuity_keywords(mod.build_parser().parse_args(["--continuity", "0"]), name, {}) == {"continuity": 0.0}
        capsys.readouterr()
        for bad, kw in ((argparse.Namespace(continuity=-1.0), {"match_width": 0.02}), (argparse.Namespace(continuity=float("nan")), {"match_width": 0.02}),
                        (argparse.Namespace(continuity=0.5), {}), (argparse.Namespace(continuity=0.5), {"match_width": float("inf")})):
            with pytest.raises(SystemExit):
                continuity_keywords(bad, name, kw)
    if "--chunked" in infer.build_parser().format_help():
        assert infer.build_parser().parse_args(["--chunked", "--continuity", "0.25", "--match-width", "0.02"]).continuity == 0.25
    for cls in (infer_streaming.BatchedStreamInfer, __import__("tinyvc_amd.module.infer", fromlist=["StreamInfer"]).StreamInfer):
        assert "continuity" in inspect.signature(cls.__init__).parameters
    from tinyvc_amd.module.infer import Generator
    assert "continuity" in inspect.signature(Generator.convert).parameters
