"""SourceNet, gemm_s2's wide column tiles and the unfused ConvNeXt path, per window and per output row against the fp64 oracle.

The rule is test_gpu_tile_edges.py's: the truth is the oracle in fp64, the yardstick is the oracle in fp32 on one thread, and for every
tensor, utterance and window (or row)

    e_gpu <= max(3e-6, 2 x the worst e_ref of that case, tensor and metric)

Measured with these inputs (test_contraction_metric_host.py asserts it), the yardstick stays below 1.0e-6 per row and 8.2e-7 per window
everywhere here, so the 3e-6 floor decides every gate.  Every case prints one `[edge]` line (profiles/contraction_edges.txt).

(a) SourceNet (run_source_net: the frame maximum of the energy, content_in through gemm_s2 with the energy / log-f0 conditioning epilogue,
    three ConvNeXt layers at 128 channels, to_amps - 15 live rows of one 32-row tile - and to_kernel - 961 rows, row 960 alone in the 31st
    tile).  So far `amps` and `kernel` met one whole-tensor relative rms of 2e-6 at T = 28, 50, 200, which `kernel` row 960 off by 1e-4
    passes.  Here both tensors are gated per 32-column window AND per output row (helpers.row_errors: in the utterance's units).  The
    inputs (helpers.sourcenet_edge_inputs) reach the relu and the log(1e-6) branch of the f0 conditioning and put each frame's energy
    maximum on the first or the last sample of the frame.

      (B, T)                        what it puts on a seam
      (1, 1), (1, 3)                every depthwise tap lands on replicate padding; GRN over one and three columns
      (3, 32) / (3, 33)             cnx1<128, 1> against <128, 2>; 96 and 99 flat columns straddle utterances in the 64-column gemm_s2 tile
                                    and in the 128-column to_kernel / to_amps tile
      (3, 43)                       129 columns: a one-column tail of the flat 128-column tile behind a tile that holds three utterances
      (2, 64) / (2, 65)             a whole tile, then a one-column tail, for cnx1 and cnx2
      (1, 127) / (1, 128) / (1, 129) the non-flat (B = 1) 128-column tile on both sides of its edge
      (1, 1024) / (1, 1025)         16 against 17 GRN tile sums: inline against grn_tiles_kernel

    (3, 43) and (1, 129) also carry the planted errors ON THE HOST (helpers.planted_errors_trip): `kernel` row 960 and `amps` row 14
    x (1 + 1e-4) must trip the row gate, + 1e-4 x rms on the last two columns of either tensor must trip the window gate.

(b) The encoder at gemm_s2 column tiles of 96, 128, 160 and 192 columns.  gemm_s2_try picks the width from the column count and the CU
    count (helpers.gemm_s2_width restates it); every shape of test_encoder_per_window_at_tile_edges has at most 1025 columns and stays on
    the 64-column tile.  The shapes come from the device's CU count (helpers.wide_tile_shapes; on 256 CUs (3, 897), (17, 241), (3, 1814),
    (2, 3361) = 2691, 4097, 5442, 6722 columns): between them ssl_out (6 row blocks) takes widths 3, 4, 5, 6 with tails of 1 .. 3
    columns, pit_out (4 row blocks) widths 3 and 4.

(c) The unfused ConvNeXt path: dwconv_ln_kernel<true>, gemm_s2 for c2 with a |max| slot on its input, grn_norm_kernel,
    grn_finalize_kernel and the SCALED gemm_s2 for c3.  A layer goes there when its LayerNorm bound sqrt(C) max|gamma| + max|beta| reaches
    32768; the synthetic checkpoints have 14 .. 26, so nothing else in the suite runs these five launches.  helpers.rescaled_ln multiplies
    gamma and beta by 2^12 and c2.weight by 2^-12 - the same function exactly, bit for bit in the fp32 oracle - and takes the bound to
    5.7e4 .. 1.05e5.  Variant A rescales every ConvNeXt layer of both estimators and of SourceNet; variant B every second one
    (mid_layers.1, .3, .5), so fused and unfused layers alternate and SourceNet's last layer publishes its |max| slot from the fused
    path, where A publishes it from the unfused one.  The truth and the yardstick come from the rescaled state dict.  Each case also
    notes whether the result equals the unrescaled checkpoint's GPU result bit for bit - not asserted: nothing derives it once the c2 input
    carries a |max| slot.  One ragged encode under variant A (3, 33, 64, 65, 130 frames) must equal every row's own B = 1 call bit for
    bit: the only run of the unfused kernels' ragged tables."""
import pytest
import torch

from helpers import (PIT_OUT_MBLOCKS, SOURCE_BUMP_SHAPES, SOURCE_SHAPES, SSL_OUT_MBLOCKS, _bump_trips, _gate_case, convnext_prefixes, gate_windows_and_rows,
                     gemm_s2_width, ln_bound, oracle_one_thread, planted_errors_trip, rel_rms, rescaled_ln, sourcenet_edge_inputs, state_dicts, wide_tile_shapes)
from oracle import ref_cpu as R
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC_TRUNKS, DEC_TRUNKS = ("ssl_feature_estimator", "pitch_estimator"), ("source_net",)
VARIANTS = {"A": "all", "B": "second"}

_CACHE = {}


def _sds(variant=None):
    """(encoder, decoder) state dicts of the synthetic checkpoint, or of its rescaled variant 'A' / 'B'."""
    if ("sd", variant) not in _CACHE:
        enc_sd, dec_sd = state_dicts(0)
        if variant is not None:
            enc_sd = rescaled_ln(enc_sd, convnext_prefixes(ENC_TRUNKS, VARIANTS[variant]))
            dec_sd = rescaled_ln(dec_sd, convnext_prefixes(DEC_TRUNKS, VARIANTS[variant]))
        _CACHE["sd", variant] = (enc_sd, dec_sd)
    return _CACHE["sd", variant]


def _sds64(variant=None):
    if ("sd64", variant) not in _CACHE:
        _CACHE["sd64", variant] = tuple({k: v.double() for k, v in sd.items()} for sd in _sds(variant))
    return _CACHE["sd64", variant]


def _gen(variant=None):
    if ("gen", variant) not in _CACHE:
        assert torch.cuda.is_available(), "gpu tests need an MI355X"
        from tinyvc_amd.module.infer import Generator
        from tinyvc_amd.module.tinyvc import Decoder, Encoder
        enc_sd, dec_sd = _sds(variant)
        enc, dec = Encoder(), Decoder()
        enc.load_state_dict(enc_sd)
        dec.load_state_dict(dec_sd)
        _CACHE["gen", variant] = Generator(enc, dec).to(DEV)
    return _CACHE["gen", variant]


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_bounds(variant):
    """The bound of pack.hip restated: >= 32768 (unfused) for exactly the rescaled layers of this variant."""
    for sd, trunks in zip(_sds(variant), (ENC_TRUNKS, DEC_TRUNKS)):
        chosen = convnext_prefixes(trunks, VARIANTS[variant]) if variant else []
        for p in convnext_prefixes(trunks):
            assert (ln_bound(sd, p) >= 32768.0) == (p in chosen), (variant, p, ln_bound(sd, p))


# ------------------------------------------------------------------------------------------------ SourceNet
def _named(amps, kern):
    return {"amps": amps, "kernel": kern}


def _source_case(case, variant, B, T, bumps):
    inp = sourcenet_edge_inputs(B, T)
    truth = _named(*R.source_net(_sds64(variant)[1], *[x.double() for x in inp]))
    with oracle_one_thread():
        ref = _named(*R.source_net(_sds(variant)[1], *inp))
    dev = [x.to(DEV) for x in inp]
    gpu = _named(*_gen(variant).decoder.engine(DEV).source_net(*dev))
    extra = ""
    if variant is not None:
        base = _named(*_gen().decoder.engine(DEV).source_net(*dev))
        same = [k for k in gpu if torch.equal(gpu[k], base[k])]
        extra = "; equal to the unrescaled checkpoint's GPU result bit for bit: " + (", ".join(same) if same else "neither tensor") + \
                "".join(f" ({k} differs by {rel_rms(gpu[k].cpu(), base[k].cpu()):.1e})" for k in gpu if k not in same)
    gpu = {k: v.cpu() for k, v in gpu.items()}
    fails, gates = gate_windows_and_rows(case, gpu, truth, ref, extra=extra)
    assert not fails, f"{case}: " + "; ".join(fails)
    if bumps:
        missed = planted_errors_trip(gpu, truth, gates)
        assert not missed, f"{case}: planted errors that did not trip their gate: " + ", ".join(missed)


@pytest.mark.parametrize("B,T", SOURCE_SHAPES)
def test_source_net_per_window_and_per_row_at_tile_edges(B, T):
    """(a)"""
    _assert_bounds(None)
    _source_case(f"source_net B={B} T={T}", None, B, T, bumps=(B, T) in SOURCE_BUMP_SHAPES)


# ------------------------------------------------------------------------------------------------ encoder at the wide gemm_s2 tiles
def _encoder_case(case, variant, B, T):
    e64, enc_sd = _sds64(variant)[0], _sds(variant)[0]
    spec = R.spectrogram(synth.synth_wave(B, 480 * T, seed=2000 + T))
    s64 = spec.double()
    truth = {"ssl": R.ssl_features(e64, s64), "logits": R.pitch_logits(e64, s64)}
    f0_truth = R.pitch_decode(truth["logits"])
    with oracle_one_thread():
        ref = {"ssl": R.ssl_features(enc_sd, spec), "logits": R.pitch_logits(enc_sd, spec)}
    sdev = spec.to(DEV)
    ssl, f0, logits = _gen(variant).encoder.engine(DEV).encoder(sdev, want_logits=True)
    gpu = {"ssl": ssl, "logits": logits}
    e_f0 = rel_rms(f0.cpu(), f0_truth)
    extra = f"; f0 rel rms vs the fp64 truth {e_f0:.2e}"
    if variant is not None:
        ssl0, f00, logits0 = _gen().encoder.engine(DEV).encoder(sdev, want_logits=True)
        base = {"ssl": ssl0, "logits": logits0, "f0": f00}
        mine = dict(gpu, f0=f0)
        same = [k for k in mine if torch.equal(mine[k], base[k])]
        extra += "; equal to the unrescaled checkpoint's GPU result bit for bit: " + (", ".join(same) if same else "no tensor") + \
                 "".join(f" ({k} differs by {rel_rms(mine[k].cpu(), base[k].cpu()):.1e})" for k in mine if k not in same)
    fails, gates = _gate_case(case, gpu, truth, ref, extra=extra)
    assert not fails, f"{case}: " + "; ".join(fails)
    assert _bump_trips(gpu, truth, gates, "ssl"), "1e-4 x rms on the last two columns of ssl must trip the window gate"
    assert _bump_trips(gpu, truth, gates, "logits"), "1e-4 x rms on the last two columns of the logits must trip the window gate"
    assert e_f0 <= 2e-6


def _wide_shapes():
    ncu = _ncu()
    shapes = wide_tile_shapes(ncu)
    if None in shapes:
        pytest.skip(f"{ncu} CUs: no B x T near the 256-CU shapes selects gemm_s2 widths 3, 4, 5 and 6 for ssl_out with a tail of 1 .. 3 columns ({shapes})")
    return ncu, shapes


def test_wide_shapes_cover_every_gemm_s2_width_on_this_device():
    """(b) the coverage the four cases below stand on, for the device they run on."""
    ncu, shapes = _wide_shapes()
    cols = [B * T for B, T in shapes]
    ssl_w = [gemm_s2_width(n, SSL_OUT_MBLOCKS, ncu) for n in cols]
    pit_w = [gemm_s2_width(n, PIT_OUT_MBLOCKS, ncu) for n in cols]
    assert ssl_w == [3, 4, 5, 6], (ncu, shapes, ssl_w)
    assert {3, 4} <= set(pit_w), (ncu, shapes, pit_w)
    tails = [n % (32 * w) for n, w in zip(cols, ssl_w)]
    assert all(1 <= t <= 3 for t in tails), (ncu, shapes, tails)
    print(f"[edge] encoder wide tiles on {ncu} CUs: shapes {shapes} = {cols} columns; ssl_out widths {ssl_w} x 32 columns with tails {tails}; pit_out widths {pit_w}")


@pytest.mark.parametrize("i", range(4))
def test_encoder_per_window_at_wide_gemm_s2_tiles(i):
    """(b) ssl_out at width 3 + i; the largest call of this file is the last one (6722 frames on 256 CUs)."""
    ncu, shapes = _wide_shapes()
    B, T = shapes[i]
    _assert_bounds(None)
    _encoder_case(f"encoder B={B} T={T} ({B * T} columns: ssl_out width {gemm_s2_width(B * T, SSL_OUT_MBLOCKS, ncu)}, pit_out width {gemm_s2_width(B * T, PIT_OUT_MBLOCKS, ncu)})",
                  None, B, T)


# ------------------------------------------------------------------------------------------------ the unfused ConvNeXt path
@pytest.mark.parametrize("B,T", [(3, 32), (3, 33), (3, 65), (1, 1025), (3, 1814)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_encoder_unfused_convnext_per_window(variant, B, T):
    """(c) both estimators with every (A) or every second (B) ConvNeXt layer on the five unfused launches.  At (3, 1814) the 384-channel
    c2 and c3 launches of gemm_s2 leave the 64-column width (on 256 CUs: 5 and 3 units of 32 columns; the 128-channel ones, 2 and 1 row
    blocks, stay at 2)."""
    _assert_bounds(variant)
    ncu = _ncu()
    w = {f"{c} ch c2 / c3": (gemm_s2_width(B * T, 2 * c // 128, ncu), gemm_s2_width(B * T, c // 128, ncu)) for c in (384, 128)}
    if (B, T) == (3, 1814) and ncu == 256:
        assert w["384 ch c2 / c3"] == (5, 3), w
    _encoder_case(f"encoder unfused ConvNeXt variant {variant} B={B} T={T} (gemm_s2 widths {w})", variant, B, T)


@pytest.mark.parametrize("B,T", [(3, 33), (3, 43), (1, 129)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_source_net_unfused_convnext_per_window_and_per_row(variant, B, T):
    """(c) SourceNet: variant A publishes the |max| slot to_amps / to_kernel read from the unfused path, variant B from the fused one."""
    _assert_bounds(variant)
    _source_case(f"source_net unfused ConvNeXt variant {variant} B={B} T={T}", variant, B, T, bumps=(B, T) in SOURCE_BUMP_SHAPES)


def test_ragged_encode_on_the_unfused_path_equals_one_call_per_utterance():
    """(c) One ragged encode under variant A: every row's ssl and f0 equal its own B = 1 stft_mag + encoder under the same checkpoint bit
    for bit (the pattern of test_ragged_encode_equals_one_call_per_utterance_and_the_oracle), whose unfused launches the cases above have
    compared with the truth."""
    frames = [3, 33, 64, 65, 130]
    _assert_bounds("A")
    eng = _gen("A").engine(DEV)
    wav = torch.zeros(len(frames), 480 * max(frames))
    for b, f in enumerate(frames):
        wav[b, :480 * f] = synth.synth_wave(1, 480 * f, seed=600 + b)[0]
    wav = wav.to(DEV)
    ssl, f0, pre = eng.encode_ragged(wav, [480 * f for f in frames])
    assert pre == [sum(frames[:b]) for b in range(len(frames) + 1)] and ssl.shape == (768, sum(frames)) and f0.shape == (sum(frames),)
    assert torch.isfinite(ssl).all() and torch.isfinite(f0).all()
    for b, f in enumerate(frames):
        one_ssl, one_f0, _lg = eng.encoder(eng.stft_mag(wav[b:b + 1, :480 * f].contiguous()))
        assert torch.equal(ssl[:, pre[b]:pre[b + 1]], one_ssl[0]), f"utterance {b} ({f} frames): ssl of the ragged encode != its own encode"
        assert torch.equal(f0[pre[b]:pre[b + 1]], one_f0[0, 0]), f"utterance {b} ({f} frames): f0 of the ragged encode != its own encode"
    print(f"[edge] ragged encode on the unfused ConvNeXt path (variant A), frames {frames}: every row's ssl and f0 equal its own B = 1 stft_mag + encoder bit for bit")
