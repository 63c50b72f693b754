"""No entry's result depends on what its workspace held, where in a page it lay, or on memory behind it (tests/helpers_workspace.py).

Every case: `want` is the Engine's ordinary call in its own grow-only workspace; then the same call once per fill word (0, a quiet NaN, all
ones, 0x7F7F7F7F - helpers_workspace.FILLS) in a workspace of exactly the measured peak between two 64 KiB guards, at page phases 0, 1, 5, 15.
Every result tensor - waves, shifts, indices, counters, the state a call advances - equals `want` BIT FOR BIT, both guards are intact, and
where the entry takes its outputs from the caller they lie between guards of their own.  A conversion's peak is its own query's
(tvc_workspace_bytes* - 4096); a match, a stage call or an index call borrows a larger query, so its peak is read from the refusal of a
zero-byte workspace (helpers_workspace.exact_peak).  profiles/workspace_first_writers.md is the audit these runs confirm: which launch
first writes every workspace buffer, and who covers what a launch writes in part.

Shapes: B = 2, T = 37 frames (L = 17760: above the 960-sample floor, no multiple of 32, across a 32-column group boundary); ragged rows of
37, 13 and 7 frames under a cap of 45 frames per batch (two batches, so the second finds the first one's bytes, and encode_ragged's packing
launch runs); an fp32 index of 129 vectors (two image tiles, the exact search) and an fp16 one of 4097 (the two-stage search: its candidate
counters, lists and overflow flags); a second engine whose every second ConvNeXt layer runs the five unfused launches.  Noise phases are
injected: nothing draws.  Each case prints one `[ws]` line."""
import ctypes
import time

import pytest
import torch

import helpers_workspace as W
from helpers import convnext_prefixes, ln_bound, rescaled_ln, state_dicts
from tinyvc_amd import _lib, spec, synth
from tinyvc_amd.engine import _names, _ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T = 2, 37
L = T * 480
RAG_FRAMES = [37, 13, 7]
RAG_CAP = 45
N_SMALL, N_BIG = 129, 4097
NAN = float("nan")


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    t0 = time.perf_counter()      # the module's wall time: from its first fixture to its last test, the weights' packing included
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    g = Generator(enc, dec).to(DEV)
    yield g
    print(f"[ws] module wall time {time.perf_counter() - t0:.1f} s")


@pytest.fixture(scope="module")
def data(gen):
    """every input, once, and left unchanged: waves, phases, the two indices with their blobs, and the stage inputs (the engine's own stage outputs)"""
    eng = gen.engine()
    d = dict(eng=eng)
    d["wav"] = synth.synth_wave(B, L, seed=611).to(DEV)
    d["angle"] = synth.synth_angle(B, T, 612).to(DEV)
    rag = synth.synth_wave(3, L, seed=613)
    for b, f in enumerate(RAG_FRAMES):
        rag[b, f * 480:] = 0
    d["rag_wav"], d["rag_lens"], d["rag_angle"] = rag.to(DEV), [f * 480 for f in RAG_FRAMES], synth.synth_angle(3, T, 614).to(DEV)
    d["idx_small"] = synth.synth_index(N_SMALL, seed=615).to(DEV)               # fp32 storage
    d["idx_big"] = synth.synth_index(N_BIG, seed=616).to(DEV).half()            # fp16 storage
    d["small"], d["big"] = eng.knn_prepare(d["idx_small"]), eng.knn_prepare(d["idx_big"])      # (blob, N)
    # the stage calls' inputs
    d["spec"] = eng.stft_mag(d["wav"])
    d["ssl"], d["f0"], d["logits"] = eng.encoder(d["spec"], want_logits=True)
    d["energy"] = eng.energy(d["wav"])
    d["amps"], d["kern"] = eng.source_net(d["ssl"], d["f0"], d["energy"])
    d["source"] = eng.dsp(d["f0"], d["amps"], d["kern"], d["angle"])
    torch.cuda.synchronize()
    return d


# ---- the scheme ---------------------------------------------------------------------------------------------------------------------------------
class Outs:
    """where a case takes its caller-owned outputs from: plain tensors for `want`, guarded ones (checked behind the block) under a fill"""

    def __init__(self, guarded):
        self.guarded, self.made = guarded, []

    def __call__(self, shape, dtype=torch.float32, fill=NAN):
        if not self.guarded:
            return torch.full(shape, fill, dtype=dtype, device=DEV)
        g = W.guarded_output(shape, dtype, fill, DEV)
        self.made.append(g)
        return g.tensor

    def check(self, what):
        for i, g in enumerate(self.made):
            bad = g.violations()
            assert not bad, f"{what}: output {i}: " + "; ".join(bad)


def run_case(name, eng, call, tight=False):
    """call(outs) -> the result tensors.  tight: the call borrows a larger query - carve the peak its zero-byte refusal names."""
    want = call(Outs(False))
    torch.cuda.synchronize()
    peak, note = None, ""
    if tight:
        peak = W.exact_peak(eng, lambda: call(Outs(False)))
        if peak is None:      # nothing to poison: the call still runs below, in a workspace of zero bytes between the guards
            peak, note = 0, " - takes no workspace (the zero-byte probe was not refused)"
    carved = []
    for word, phase in zip(W.FILLS, W.PHASES):
        outs = Outs(True)
        with W.guarded_workspace(eng, word, phase, peak=peak) as g:
            got = call(outs)
        what = f"{name} under fill {word:#010x} at phase {phase}"
        outs.check(what)
        W.assert_same_bits(got, want, what)
        carved = g.peaks
    print(f"[ws] {name}: carved peak {'+'.join(str(p) for p in carved) if carved else 0} bytes{note}, {len(W.FILLS)} fills passed"
          f"{', outputs guarded' if outs.made else ''}")


def ragged_cap(eng):
    class Cap:
        def __enter__(self):
            eng.set_ragged_batch_frames(RAG_CAP)

        def __exit__(self, *exc):
            eng.set_ragged_batch_frames(0)
    return Cap()


def floats(vals):
    return torch.tensor(vals, dtype=torch.float32, device=DEV)


# ---- conversions: every form of Engine._convert ----------------------------------------------------------------------------------------------------
def _index(d, form, rows):
    """(prepared, Ns, weights) of a call of `rows` rows: shared = the big index; else the two indices alternating (a blend: both per row)"""
    (bs, ns), (bb, nb) = d["small"], d["big"]
    if form.startswith("shared"):
        return (bs, ns, None) if form.endswith("small") else (bb, nb, None)
    if form == "blend":
        return [bs, bb] * rows, [ns, nb] * rows, floats([[0.25, 0.75]] * rows)
    alt = [(bs, ns), (bb, nb)]
    return [alt[r % 2][0] for r in range(rows)], [alt[r % 2][1] for r in range(rows)], None


CONVERSIONS = ["shared-small", "shared-big", "multi", "blend", "auto", "alpha", "protect", "path"]


def _convert_case(d, form, ragged):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchCarry, PitchPath, PitchTrack
    eng = d["eng"]
    rows = 3 if ragged else B
    wav, angle, lens = (d["rag_wav"], d["rag_angle"], d["rag_lens"]) if ragged else (d["wav"], d["angle"], None)
    prepared, ns, weights = _index(d, form, rows)
    shifts = [2.0, -3.0, 1.0][:rows]
    target = floats([150.0, 220.0, 180.0][:rows])
    alpha, protect = floats([0.25, 0.6, 0.0][:rows]), floats([0.5, 1.0, 0.75][:rows])
    start = torch.linspace(-30.0, 0.0, 512, device=DEV).repeat(rows, 1).contiguous()      # a carried state that is not the fresh one

    def call(outs):
        out = outs((rows, L))
        if form.startswith("shared"):
            return eng._convert("shared", wav, prepared, ns, 0.5, angle, lens, out=out)
        if form in ("multi", "blend"):
            return eng._convert("table" if form == "multi" else "blend", wav, prepared, ns, shifts, angle, lens, weights, out=out)
        if form == "auto":
            return eng._convert("auto", wav, prepared, ns, shifts, angle, lens, None, target, out=out, shift_out=outs((rows,)))
        if form == "alpha":
            return eng._convert("alpha", wav, prepared, ns, shifts, angle, lens, alpha=alpha, out=out)
        if form == "protect":
            return eng._convert("protect", wav, prepared, ns, shifts, angle, lens, alpha=alpha, protect=protect, out=out)
        if form == "path":      # the default path with alpha, protect and target registers: lgt, bp, share, srcmax, abound, rowmax all exist at once
            return eng._convert("path", wav, prepared, ns, shifts, angle, lens, None, target, out=out, shift_out=outs((rows,)), alpha=alpha, protect=protect, path=PitchPath())
        if form == "path-carry":      # the state is the call's too: every call starts from the same one and leaves the same one
            carry = PitchCarry(rows, 4, device=DEV)
            carry.scores.copy_(start)
            res = eng._convert("path", wav, prepared, ns, shifts, angle, None, None, target, out=out, shift_out=outs((rows,)), alpha=alpha, protect=protect,
                               path=PitchPath(), carry=carry)
            return res, carry.scores
        if form == "track":
            track = PitchTrack(rows, 4, lag_frames=8, window_frames=8, min_voiced=1, device=DEV)
            res = eng._convert("track", wav, prepared, ns, shifts, angle, None, None, target, out=out, shift_out=outs((rows,)), track=track)
            return res, track.ring, track.count, track.auto
        raise AssertionError(form)
    return call


@pytest.mark.parametrize("form", CONVERSIONS + ["path-carry", "track"])
def test_equal_length_conversions(data, form):
    run_case(f"convert {form}", data["eng"], _convert_case(data, form, False))


@pytest.mark.parametrize("form", CONVERSIONS)
def test_ragged_conversions(data, form):
    with ragged_cap(data["eng"]):
        run_case(f"convert_ragged {form}", data["eng"], _convert_case(data, form, True))


# ---- matches ---------------------------------------------------------------------------------------------------------------------------------------
def _match(eng, form, src, prepared, Ns, outs, weights=None, alpha=None, f0=None, protect=None):
    """Engine._match with the caller's `matched` and `idx`: the same arguments under the C parameters' names, the outputs from `outs`"""
    Bm, _, Tm = src.shape
    named, sized = eng._index_args(form, prepared, Ns, weights, Bm)
    named.update(src=_ptr(src), B=Bm, T=Tm)
    if form in ("alpha", "protect"):
        named["alpha"] = _ptr(alpha)
    if form == "protect":
        named["protect"], named["f0"] = _ptr(protect), _ptr(f0)
    terms = (sized["M"],) if "M" in sized else ()
    out = outs((Bm, spec.SSL_DIM, Tm))
    idx = outs((*terms, Bm, Tm, 4), torch.int64, -7)
    query, entry = _names(form)
    named["ws"], named["ws_bytes"] = eng._query_ws(query, B=Bm, L=Tm * spec.HOP, **sized)
    named.update(ctx=eng.ctx, stream=eng._stream(), out=_ptr(out), idx_out=_ptr(idx))
    eng._ok(getattr(eng.lib, entry)(*_lib.arguments(entry, named)), entry)
    return out, idx


MATCHES = ["match", "match_multi", "match_blend", "match_alpha", "match_protect", "topk-gather-finish", "match_general"]


@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("form", MATCHES)
def test_matches(data, form, which):
    d, eng = data, data["eng"]
    src, f0 = d["ssl"], d["f0"]
    blob, n = d[which]
    other = d["big" if which == "small" else "small"]
    table, tns = [blob, other[0]], [n, other[1]]      # this index first, the other on the second row (a blend: both per row)
    alpha, protect = floats([0.25, 0.6]), floats([0.5, 1.0])
    weights = floats([[0.25, 0.75]] * B)

    def call(outs):
        if form == "match":
            return _match(eng, "shared", src, blob, n, outs)
        if form == "match_multi":
            return _match(eng, "table", src, table, tns, outs)
        if form == "match_blend":
            return _match(eng, "blend", src, table * B, tns * B, outs, weights)
        if form == "match_alpha":
            return _match(eng, "alpha", src, table, tns, outs, alpha=alpha)
        if form == "match_protect":
            return _match(eng, "protect", src, table, tns, outs, alpha=alpha, f0=f0, protect=protect)
        if form == "topk-gather-finish":
            sims, idx = eng.knn_topk(src, blob, n)
            slots = eng.knn_gather_slots(blob, n, idx)
            return sims, idx, slots, eng.knn_finish(slots)
        raw = (d["idx_small"] if which == "small" else d["idx_big"].float())[0].contiguous()      # the raw index: plain fp32, k = 5, L2
        return eng.knn_match_general(src, raw, 5, "L2", want_indices=True)
    run_case(f"{form} N={n}", eng, call, tight=True)


# ---- stage calls -----------------------------------------------------------------------------------------------------------------------------------
def _encode_ragged(d, outs):
    eng = d["eng"]
    lens = eng._lens(d["rag_lens"], 3)
    S = sum(RAG_FRAMES)
    ssl, f0 = outs((spec.SSL_DIM, S)), outs((S,))
    p, n = eng._query_ws("tvc_workspace_bytes_encode_ragged", 3, L, lens)
    eng._ok(eng.lib.tvc_encode_ragged_f32(eng.ctx, eng._stream(), _ptr(d["rag_wav"]), L, lens, _ptr(ssl), _ptr(f0), 3, p, n), "tvc_encode_ragged_f32")
    return ssl, f0


def _pitch_path_rows(d, outs):
    """two rows of unequal length in one packed logits tensor: 37 and 13 frames of 74 columns (the rest belong to no row and read 0)"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath
    packed = d["logits"].permute(1, 0, 2).reshape(spec.PITCH_CLASSES, B * T).contiguous()
    return d["eng"].pitch_path(packed, PitchPath(), row_start=[0, 37, 50], pitch_shift=[2.0, -3.0], want_shifted=True)


STAGES = {
    "stft_mag": lambda d, outs: d["eng"].stft_mag(d["wav"]),
    "energy": lambda d, outs: d["eng"].energy(d["wav"]),
    "energy L=17953": lambda d, outs: d["eng"].energy(d["odd_wav"]),      # no whole number of frames, nor of the 64-sample pooling stride
    "encoder+logits": lambda d, outs: d["eng"].encoder(d["spec"], want_logits=True),
    "decoder stages": lambda d, outs: d["eng"].decoder(d["ssl"], d["f0"], d["energy"], d["angle"], stages=True),
    "source_net": lambda d, outs: d["eng"].source_net(d["ssl"], d["f0"], d["energy"]),
    "filter_net blocks": lambda d, outs: d["eng"].filter_net(d["ssl"], d["f0"], d["energy"], d["source"], blocks=True),
    "dsp": lambda d, outs: d["eng"].dsp(d["f0"], d["amps"], d["kern"], d["angle"]),
    "pitch_path rows 37+13": _pitch_path_rows,
    "encode_ragged": _encode_ragged,
}


@pytest.mark.parametrize("stage", list(STAGES))
def test_stage_calls(data, stage):
    d = data
    if "odd_wav" not in d:
        d["odd_wav"] = synth.synth_wave(B, 17953, seed=617).to(DEV)
    with ragged_cap(d["eng"]):
        run_case(stage, d["eng"], lambda outs: STAGES[stage](d, outs), tight=True)


# ---- the unfused ConvNeXt launches ------------------------------------------------------------------------------------------------------------------
# A ConvNeXt layer whose LayerNorm bound (pack.hip: sqrt(C) max|gamma| + max|beta|) reaches 32768 leaves the two fused launches for
# run_convnext's five, with workspace of their own: y, the GRN factors nx, and the |max| slots ymax (its own memset) and hmax.  The synthetic
# checkpoint has bounds of 14 .. 26, so nothing above runs them; helpers.rescaled_ln moves every second layer there (the same function exactly).
@pytest.fixture(scope="module")
def unfused(data):
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    chosen = {}
    for name, sd, trunks in (("enc", enc_sd, ("ssl_feature_estimator", "pitch_estimator")), ("dec", dec_sd, ("source_net",))):
        picked = convnext_prefixes(trunks, "second")
        chosen[name] = rescaled_ln(sd, picked)
        for pre in convnext_prefixes(trunks):
            assert (ln_bound(chosen[name], pre) >= 32768.0) == (pre in picked), (pre, ln_bound(chosen[name], pre))
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(chosen["enc"])
    dec.load_state_dict(chosen["dec"])
    g = Generator(enc, dec).to(DEV)
    return dict(data, eng=g.engine(), gen=g)      # the same inputs and blobs, this engine's weights and workspace


@pytest.mark.parametrize("case", ["convert path", "convert_ragged path", "encoder+logits", "source_net", "encode_ragged"])
def test_unfused_convnext_layers(unfused, case):
    d = unfused
    with ragged_cap(d["eng"]):
        if case.startswith("convert"):
            run_case(f"{case}, every second ConvNeXt layer unfused", d["eng"], _convert_case(d, "path", case.startswith("convert_ragged")))
        else:
            run_case(f"{case}, every second ConvNeXt layer unfused", d["eng"], lambda outs: STAGES[case](d, outs), tight=True)


# ---- index work ------------------------------------------------------------------------------------------------------------------------------------
IC_N, IC_K, IC_ITERS = 300, 8, 2


@pytest.fixture(scope="module")
def points(data):
    eng = data["eng"]
    blob, n = eng.knn_prepare(synth.synth_index(IC_N, seed=618).to(DEV))
    cols = (torch.arange(IC_K, dtype=torch.int64) * 37).to(DEV)
    index, cblob, assign, _counts, _moved = eng.index_compact(blob, n, cols, IC_ITERS)
    torch.cuda.synchronize()
    return dict(blob=blob, cols=cols, cblob=cblob, assign=assign, index=index)


@pytest.mark.parametrize("which", ["index_assign", "index_update", "index_compact"])
def test_index_work(data, points, which):
    eng, p = data["eng"], points
    q = data["ssl"][:1].contiguous()

    def call(outs):
        if which == "index_assign":
            return eng.index_assign(p["blob"], IC_N, p["cblob"], IC_K)                      # (assign, sims, moved); a fresh assignment every call
        if which == "index_update":
            return eng.index_update(p["blob"], IC_N, p["assign"], p["index"][0].clone())     # (centroids, counts); the centroids are the call's to update
        index, blob, assign, counts, moved = eng.index_compact(p["blob"], IC_N, p["cols"], IC_ITERS)
        return index, assign, counts, moved, eng.knn_topk(q, blob, IC_K)                     # the blob through a search
    run_case(f"{which} N={IC_N} K={IC_K}", eng, call, tight=True)


def _blob_words(blob):
    return blob[:64].view(torch.int32).cpu()


@pytest.mark.parametrize("kind", ["prepare_f32", "prepare_f16", "columns_f32", "columns_f16"])
def test_prepare_writes_a_whole_blob_into_poisoned_memory(data, kind):
    """knn_prepare / knn_prepare_columns through the C ABI into a destination that held each fill word, between guards: the header's words
    beyond BLOB_WORDS read zero (knn_blob.h: "the rest is zero") and a search through the blob equals the search through the Engine's own."""
    eng, lib = data["eng"], data["eng"].lib
    half = kind.endswith("f16")
    q = data["ssl"]
    if kind.startswith("prepare"):
        index = data["idx_big"] if half else data["idx_small"]
        N = index.shape[2]
        rows = index[0].t().contiguous() if half else index[0].contiguous()
        w_blob = data["big" if half else "small"][0]

        def prepare(dst):
            entry = "tvc_knn_prepare_index_f16" if half else "tvc_knn_prepare_index_f32"
            eng._ok(getattr(lib, entry)(eng.ctx, eng._stream(), _ptr(rows), _ptr(dst), N), entry)
    else:
        feats = torch.cat([data["idx_small"][0], data["idx_big"][0, :, :171].float()], dim=1).contiguous()      # [768, 300] packed features
        S, N = feats.shape[1], N_SMALL
        cols = ((torch.arange(N, dtype=torch.int64) * 7) % S).to(DEV)
        w_blob, _n, w_index = eng.knn_prepare_columns(feats, cols, half=half)
        w_index = w_index.clone()

        def prepare(dst):
            entry = "tvc_knn_prepare_index_cols_f16" if half else "tvc_knn_prepare_index_cols_f32"
            index = torch.full((1, spec.SSL_DIM, N), NAN, dtype=torch.float16 if half else torch.float32, device=DEV)
            eng._ok(getattr(lib, entry)(eng.ctx, eng._stream(), _ptr(feats), S, _ptr(cols), N, _ptr(dst), _ptr(index)), entry)
            assert W.same_bits(index, w_index), "index_out"
    elems = lib.tvc_knn_prepared_elems_f16(N) if half else lib.tvc_knn_prepared_elems(N)
    assert w_blob.numel() == elems
    want = eng.knn_topk(q, w_blob, N)
    torch.cuda.synchronize()
    for word in W.FILLS:
        dst = W.guarded_output((elems,), torch.float32, 0.0, DEV)
        W.fill_words(dst.arena.body, word)
        try:
            prepare(dst.tensor)
            torch.cuda.synchronize()
            dst.check()
            words = _blob_words(dst.tensor)
            assert not words[6:].any(), f"fill {word:#010x}: header words beyond BLOB_WORDS = 6 are {words[6:].tolist()}"
            assert torch.equal(words[:4], _blob_words(w_blob)[:4]) and int(words[5]) == int(_blob_words(w_blob)[5])
            assert W.same_bits(dst.tensor[4:5], w_blob[4:5]), f"fill {word:#010x}: the |max| word"
            W.assert_same_bits(eng.knn_topk(q, dst.tensor, N), want, f"{kind}: a search through the blob under fill {word:#010x}")
            torch.cuda.synchronize()
        finally:
            lib.tvc_knn_forget(eng.ctx, ctypes.c_void_p(dst.tensor.data_ptr()))      # the arena's address will be reused (Engine._owned)
    print(f"[ws] {kind} N={N}: no workspace, a destination of {elems * 4} bytes between guards, {len(W.FILLS)} fills passed")
