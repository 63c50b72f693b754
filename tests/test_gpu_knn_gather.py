"""The four routes from top-4 lists to `matched` (csrc/knn_gather.hip) against one torch restatement, bit for bit.

The routes share the list merge, the four-row gather, the mean and the transposed store; this file drives each of them at the shapes
where those shared pieces can go wrong - a lone column, 32-column groups that end mid-group and straddle a row (and, with one index
per row, a segment) boundary - with an index the exact kernel searches alone (N = 129: two image tiles) and one the two-stage search
takes (N = 4097), in both storages and mixed.  The restatement takes the indices a call returned (the search's own correctness is
tested in test_gpu_parity.py and is not restated here): rows = index[:, idx] in fp32 (fp16 storage: of index.half().float()),
mu = (((r0 + r1) + r2) + r3) * 0.25 as separate fp32 operations on the CPU, a blend = w0 * mu0, then + w1 * mu1.  No tolerance anywhere."""
import pytest
import torch

from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (129, 4097)
SHAPES = [(1, 1), (2, 33), (3, 65)]                                   # 1, 66 and 195 query columns
KINDS = [("f32", "f32"), ("f16", "f16"), ("f32", "f16")]              # storage of the two indices


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


@pytest.fixture(scope="module")
def indices(eng):
    """(size, storage) -> (the raw vectors the gather must return [768, N] fp32 on the CPU, prepared blob, N); read-only"""
    out = {}
    for i, n in enumerate(SIZES):
        index = synth.synth_index(n, seed=61 + i)
        for kind in ("f32", "f16"):
            stored = index.half() if kind == "f16" else index
            blob, nn = eng.knn_prepare(stored.to(DEV))
            out[(n, kind)] = (stored.float()[0], blob, nn)
    return out


def _mean4(rows, idx):
    """rows [768, N], idx [T, 4] -> [768, T]: (((r0 + r1) + r2) + r3) * 0.25, every operation rounded on its own"""
    r = rows[:, idx.cpu()]                                            # [768, T, 4]
    s = torch.add(torch.add(torch.add(r[..., 0], r[..., 1]), r[..., 2]), r[..., 3])
    return torch.mul(s, 0.25)


@pytest.mark.parametrize("kinds", KINDS, ids=lambda k: "+".join(k))
@pytest.mark.parametrize("B,T", SHAPES)
def test_every_route_equals_the_restatement(eng, indices, B, T, kinds):
    two = [indices[(n, k)] for n, k in zip(SIZES, kinds)]
    src = torch.randn(B, 768, T, generator=torch.Generator().manual_seed(100 * B + T)).to(DEV)

    # (a) one index for the whole call, and (d) the sharded route's three steps on it: the same bits, indices included
    for rows, blob, n in two:
        out, idx = eng.knn_match(src, blob, n, want_indices=True)
        assert idx.shape == (B, T, 4) and int(idx.min()) >= 0 and int(idx.max()) < n
        want = torch.stack([_mean4(rows, idx[b]) for b in range(B)])
        assert torch.equal(out.cpu(), want), f"knn_match, N = {n}"
        sims, tidx = eng.knn_topk(src, blob, n)
        assert torch.equal(tidx, idx), f"knn_topk indices, N = {n}"
        fin = eng.knn_finish(eng.knn_gather_slots(blob, n, tidx))
        assert torch.equal(fin, out), f"topk -> slots -> finish, N = {n}"

    # (b) one index per row, alternating: the restatement, and every row its own B = 1 call of (a)
    per_row = [two[b % 2] for b in range(B)]
    blobs, ns = [p[1] for p in per_row], [p[2] for p in per_row]
    multi, midx = eng.knn_match_multi(src, blobs, ns, want_indices=True)
    for b in range(B):
        assert torch.equal(multi[b].cpu(), _mean4(per_row[b][0], midx[b])), f"knn_match_multi, row {b}"
        one, oidx = eng.knn_match(src[b:b + 1].contiguous(), blobs[b], ns[b], want_indices=True)
        assert torch.equal(midx[b], oidx[0]) and torch.equal(multi[b], one[0]), f"row {b} differs from its own call"

    # (c) a blend: M = 1, weight 1 is (b) ...
    ones = torch.ones(B, 1, device=DEV)
    out, idx = eng.knn_match_blend(src, blobs, ns, ones, want_indices=True)
    assert torch.equal(out, multi) and torch.equal(idx[0], midx)
    # ... and M = 2, weights (0.25, 0.75): term 0 of row b is row b's index, term 1 the other one
    w = torch.tensor([[0.25, 0.75]] * B, device=DEV)
    terms = [[two[(b + m) % 2] for m in range(2)] for b in range(B)]
    out, idx = eng.knn_match_blend(src, [t[1] for row in terms for t in row], [t[2] for row in terms for t in row], w, want_indices=True)
    assert idx.shape == (2, B, T, 4)
    assert torch.equal(idx[0], midx), "term 0 is the multi-index call's search"
    for b in range(B):
        mu0, mu1 = _mean4(terms[b][0][0], idx[0, b]), _mean4(terms[b][1][0], idx[1, b])
        want = torch.mul(mu0, 0.25)
        want = torch.add(want, torch.mul(mu1, 0.75))
        assert torch.equal(out[b].cpu(), want), f"knn_match_blend, row {b}"
