"""The weighted match (tvc_knn_match_weighted_f32, tvc_weighted_convert_f32, tvc_weighted_convert_ragged_f32; Generator.convert(k=, match_width=))
without a GPU: the definition's consequences on its numpy restatement (tests/helpers_match_weight.py), the symbols, the refusals of the
Python layer and the entry scripts' arguments."""
import argparse
import itertools

import numpy as np
import pytest
import torch

from tinyvc_amd import _lib

import helpers_match_weight as mw

F = np.float32
NEW = ["tvc_knn_match_weighted_f32", "tvc_weighted_convert_f32", "tvc_weighted_convert_ragged_f32"]


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


@pytest.fixture(scope="module")
def columns():
    """40 columns: sorted similarities with gaps of every size, rows with a -0.0 and a denormal-free spread of magnitudes"""
    rng = np.random.default_rng(3)
    sims = np.sort(rng.uniform(0.2, 0.9, (40, 4)).astype(F), axis=1)[:, ::-1].copy()
    sims[:8, 1:] = sims[:8, :1] - rng.uniform(0, 0.01, (8, 3)).astype(F).cumsum(axis=1)      # near neighbours: weights inside (0, 1)
    rows = (rng.standard_normal((64, 24)) * np.exp(rng.uniform(-3, 3, (64, 1)))).astype(F)
    rows[:, 5] = F(-0.0)
    idx = np.stack([rng.permutation(64)[:4] for _ in range(40)])
    return sims, idx, rows


# ---- the definition's consequences -----------------------------------------------------------------------------------------------------
def test_k4_infinite_width_is_the_flat_mean_by_bits(columns):
    sims, idx, rows = columns
    assert np.array_equal(bits(mw.match(sims, idx, rows, 4, np.inf)), bits(mw.mean4(rows[idx])))


def test_k2_infinite_width_is_half_the_sum_by_bits(columns):
    sims, idx, rows = columns
    r = rows[idx]
    assert np.array_equal(bits(mw.match(sims, idx, rows, 2, np.inf)), bits(((r[:, 0] + r[:, 1]).astype(F) * F(0.5)).astype(F)))


def test_k1_and_width_0_without_ties_give_the_nearest_rows_own_bits(columns):
    sims, idx, rows = columns
    assert (np.diff(sims, axis=1) < 0).all()      # no ties
    nearest = rows[idx[:, 0]]
    assert np.signbit(nearest[:, 5]).all()        # the -0.0 element
    for k, width in ((1, np.inf), (1, 0.02), (4, 0.0), (3, 0.0)):
        assert np.array_equal(bits(mw.match(sims, idx, rows, k, width)), bits(nearest)), (k, width)


def test_ties_under_width_0_share_equally(columns):
    _, idx, rows = columns
    sims = np.tile(np.array([0.75, 0.75, 0.5, 0.25], F), (40, 1))
    w, W = mw.weights(sims, 4, 0.0)
    assert np.array_equal(w, np.tile(np.array([1, 1, 0, 0], F), (40, 1))) and (W == 2).all()
    r = rows[idx]
    assert np.array_equal(bits(mw.match(sims, idx, rows, 4, 0.0)), bits(((r[:, 0] + r[:, 1]).astype(F) / F(2)).astype(F)))
    sims[:] = F(0.5)      # all four tie
    assert np.array_equal(bits(mw.match(sims, idx, rows, 4, 0.0)), bits(mw.mean4(r)))


def test_the_rule_is_total():
    """NaN / +-inf similarities and NaN / negative widths give uniform weights over the first k; nothing divides by zero"""
    inf, nan = F(np.inf), F(np.nan)
    odd_sims = [[inf, inf, inf, inf], [inf, 0.5, 0.25, 0.0], [nan, nan, nan, nan], [0.5, 0.25, nan, -inf], [inf, inf, 0.5, -inf]]
    for s, k in itertools.product(odd_sims, (1, 2, 3, 4)):
        for width in (inf, nan, F(-1.0)):
            w, W = mw.weights(np.array([s], F), k, width)
            assert w[0].tolist() == [1.0] * k + [0.0] * (4 - k) and W[0] == k, (s, k, width)
    for width in (nan, F(-1.0), F(-0.0), -inf):      # on ordinary similarities too
        w, W = mw.weights(np.array([[0.9, 0.8, 0.7, 0.6]], F), 4, width)
        assert w[0].tolist() == [1.0] * 4 and W[0] == 4, width
    for s in odd_sims + [[0.9, 0.8, 0.7, 0.6]]:      # any width at all: weights in [0, 1], W in [1, k]
        for width, k in itertools.product((F(0), F(1e-30), F(0.05), F(1e30), inf, nan, F(-3)), (-7, 0, 1, 3, 4, 1000)):
            w, W = mw.weights(np.array([s], F), k, width)
            kk = min(max(k, 1), 4)
            assert ((w >= 0) & (w <= 1)).all() and w[0, 0] == 1 and 1 <= W[0] <= kk and (w[0, kk:] == 0).all(), (s, width, k)
    rows = np.array([[1.0, nan], [2.0, inf], [3.0, 4.0], [5.0, 6.0]], F)      # a neighbour of weight 0 takes no part, whatever it holds
    mu = mw.match(np.array([[0.9, 0.5, 0.4, 0.3]], F), np.array([[2, 0, 1, 3]]), rows, 4, 0.1)
    assert np.array_equal(bits(mu), bits(rows[2:3]))


def test_weights_fall_with_the_rank_and_their_sum_lies_in_1_k(columns):
    sims, _, _ = columns
    for k, width in itertools.product((1, 2, 3, 4), (0.0, 0.005, 0.02, 0.3, np.inf)):
        w, W = mw.weights(sims, k, width)
        assert (np.diff(w, axis=1) <= 0).all() and (W >= 1).all() and (W <= k).all(), (k, width)
    w, _ = mw.weights(sims, 4, 0.02)
    assert ((w > 0) & (w < 1)).any() and (w == 0).any()      # the columns do reach the inside of the ramp and its end


def test_the_point_a_planted_row_comes_back_whole():
    """the index holds row A, the query is A plus small noise, the three other neighbours lie near 0.3 cosine: the flat mean of four is far from
    A; width 0.1 and k = 1 return A's bits"""
    rows, q, a = mw.planted_index()
    cos = (rows @ q) / (np.linalg.norm(rows, axis=1) * np.linalg.norm(q))
    order = np.argsort(-cos, kind="stable")[:4]
    sims, idx = cos[order].astype(F)[None], order[None]
    assert idx[0, 0] == a and sims[0, 0] > 0.95 and (np.abs(sims[0, 1:] - 0.3) < 0.05).all()
    flat = mw.match(sims, idx, rows)
    assert np.linalg.norm(flat[0] - rows[a]) > 0.5      # |A / 4 + ... - A|: most of A is gone
    for k, width in ((4, 0.1), (1, np.inf)):
        assert np.array_equal(bits(mw.match(sims, idx, rows, k, width)[0]), bits(rows[a])), (k, width)


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
    # each fused entry is its tuned sibling's argument list plus neighbours and width, behind protect
    for name, sibling in (("tvc_weighted_convert_f32", "tvc_tuned_convert_f32"), ("tvc_weighted_convert_ragged_f32", "tvc_tuned_convert_ragged_f32")):
        args, sib = _names(decl, name), _names(decl, sibling)
        at = args.index("neighbours")
        assert args[at - 1] == "protect" and args[at + 1] == "width" and args[:at] + args[at + 2:] == sib, name
        assert _lib.SIGNATURES[name][1][:at] + _lib.SIGNATURES[name][1][at + 2:] == _lib.SIGNATURES[sibling][1], name
    # the stage call: the protect stage call plus neighbours and width behind protect, and sims_out behind idx_out
    args = _names(decl, "tvc_knn_match_weighted_f32")
    assert args[args.index("neighbours") - 1] == "protect" and args[args.index("width") - 1] == "neighbours" and args[args.index("sims_out") - 1] == "idx_out"
    assert [a for a in args if a not in ("neighbours", "width", "sims_out")] == _names(decl, "tvc_knn_match_protect_f32")
    # argument checks come before any device work: no context, no call
    assert lib.tvc_knn_match_weighted_f32(*([None] * 6), 1, *([None] * 8), 1, 1, None, 0) == -1
    from tinyvc_amd import engine
    assert callable(engine.Engine.knn_match_weighted)
    # no workspace query of their own: the tuned entries', the protect match's
    assert engine._names("weighted", False) == ("tvc_workspace_bytes_path", "tvc_weighted_convert_f32")
    assert engine._names("weighted", True) == ("tvc_workspace_bytes_ragged_path", "tvc_weighted_convert_ragged_f32")
    assert engine._names("weighted") == ("tvc_workspace_bytes_protect", "tvc_knn_match_weighted_f32")
    assert engine._FEATURES_OFF["neighbours"] is None and engine._FEATURES_OFF["width"] is None


def test_k_and_width_are_normalised_on_the_host():
    from tinyvc_amd.module.tinyvc.feature_retrieval import match_k_rows, match_width_rows, resolve_match_k, resolve_match_width
    assert resolve_match_k(2, 3) == [2, 2, 2] and resolve_match_k([1, 4, 3], 3) == [1, 4, 3] and resolve_match_k((1,), 2) == [1, 1]
    rows = match_k_rows(resolve_match_k([1, 4, 3], 3), 3, "cpu")
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.tolist() == [1, 4, 3]
    for bad, why in ((0, "1 .. 4"), (5, "1 .. 4"), (-1, "1 .. 4"), (2.0, "k"), (True, "k"), ("2", "k"), ([1, 2], "2 values for a batch of 3"), ([1, 9, 1], "1 .. 4"),
                     (torch.ones(3, dtype=torch.int32), "lives on the GPU"), (torch.ones(3, dtype=torch.int64), "int32"), (torch.ones(2, dtype=torch.int32), "1 or B = 3")):
        with pytest.raises(ValueError, match=why):
            resolve_match_k(bad, 3)
    assert resolve_match_width(0.02, 2) == [0.02, 0.02] and resolve_match_width([0, float("inf")], 2) == [0.0, float("inf")]
    rows = match_width_rows(resolve_match_width([0.5, float("inf")], 2), 2, "cpu")
    assert rows.dtype == torch.float32 and rows.tolist() == [0.5, float("inf")]
    for bad, why in ((-0.1, ">= 0"), (float("nan"), ">= 0"), ([0.1, -1.0], ">= 0"), ("0.1", "match_width"), (True, "match_width"), ([0.1] * 3, "3 shares for a batch of 2"),
                     (torch.zeros(2), "lives on the GPU"), (torch.zeros(2, dtype=torch.float64), "fp32")):
        with pytest.raises(ValueError, match=why):
            resolve_match_width(bad, 2)


@pytest.fixture(scope="module")
def cpu_gen():
    """a Generator that never left the CPU: whatever reaches its engine raises TinyVCError (a RuntimeError), never ValueError"""
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_refusals_come_before_device_work(cpu_gen):
    wf = torch.zeros(2, 4800)
    plain = torch.zeros(1, 768, 8)
    for bad in (0, 5, 2.0, [1, 2, 3], "2", True, torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="k"):
            cpu_gen.convert(wf, plain, 0.0, k=bad)
    for bad in (-0.5, float("nan"), [0.1, 0.2, 0.3], "0.1", torch.zeros(2)):
        with pytest.raises(ValueError, match="match_width"):
            cpu_gen.convert(wf, plain, 0.0, match_width=bad)
    with pytest.raises(ValueError, match="match_width"):
        cpu_gen.convert(wf, [plain, plain], [0.0, 1.0], k=[1, 2], match_width=-1.0, lengths=[4800, 2400], alpha=0.5)
    # a well-formed call gets as far as the device - and there is none; None never looks at either
    for kw in (dict(k=2), dict(match_width=0.02), dict(k=[1, 4], match_width=[0.0, float("inf")]), dict(k=None, match_width=None)):
        with pytest.raises(_lib.TinyVCError):
            cpu_gen.convert(wf, plain, 0.0, **kw)
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    with pytest.raises(ValueError, match="k"):
        BatchedStreamInfer(cpu_gen, n_streams=2, k=7, device="cuda")
    with pytest.raises(ValueError, match="match_width"):
        BatchedStreamInfer(cpu_gen, n_streams=2, match_width=-0.01, device="cuda")
    with pytest.raises(ValueError, match="k"):
        StreamInfer(cpu_gen, k=0)
    st = BatchedStreamInfer(cpu_gen, n_streams=2, device="cuda")
    assert st.k is None and st.match_width is None


def test_entry_scripts_parse_k_and_width_and_leave_the_call_alone_without_them(capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.tinyvc.feature_retrieval import match_weight_keywords
    for mod, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        absent = mod.build_parser().parse_args([])
        assert absent.k is None and absent.match_width is None
        assert match_weight_keywords(absent, name) == {} and capsys.readouterr().out == ""      # nothing added to the call, nothing printed
        given = mod.build_parser().parse_args(["-k", "2", "--match-width", "0.02"])
        assert match_weight_keywords(given, name) == {"k": 2, "match_width": 0.02}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "2" in out and "0.02" in out
        assert match_weight_keywords(mod.build_parser().parse_args(["-k", "1"]), name) == {"k": 1}
        assert match_weight_keywords(mod.build_parser().parse_args(["--match-width", "inf"]), name) == {"match_width": float("inf")}
        capsys.readouterr()
        for bad in (argparse.Namespace(k=0, match_width=None), argparse.Namespace(k=5, match_width=None), argparse.Namespace(k=None, match_width=-1.0),
                    argparse.Namespace(k=None, match_width=float("nan"))):
            with pytest.raises(SystemExit):
                match_weight_keywords(bad, name)
    if "--chunked" in infer.build_parser().format_help():
        assert infer.build_parser().parse_args(["--chunked", "-k", "3"]).k == 3
    import inspect
    for cls in (infer_streaming.BatchedStreamInfer, __import__("tinyvc_amd.module.infer", fromlist=["StreamInfer"]).StreamInfer):
        params = inspect.signature(cls.__init__).parameters
        assert "k" in params and "match_width" in params
