"""The gates, inputs and shape rules of test_gpu_contraction_edges.py, proved with the oracle alone (no GPU).

SourceNet at every shape of that file: the oracle's own fp32 evaluation passes the window and the row gate, its worst figure stays below half
the 3e-6 floor - so the floor, not the yardstick, decides every SourceNet gate - and each planted error trips its gate.  The encoder at the four
wide-tile shapes likewise.  The rescaled checkpoints compute the same function bit for bit in the oracle, the restated LayerNorm bound is
>= 32768 for exactly the rescaled layers, and the restated width rule selects what the GPU file relies on at 256 CUs.

One planted error cannot trip, by the metric's design: at (B, T) = (1, 1) the only frame is unvoiced (f0 = -5), and there `amps` row 14 lies
in ELU's tail - 0.5 % of the utterance's rms - so the row x (1 + 1e-4) reads 4.7e-7 in the utterance's units, below the floor.  The same row on
its own scale is where the fp32 oracle itself reads 5e-3 (helpers.row_errors); the test pins the arithmetic of that one case instead."""
import pytest
import torch

from helpers import (CONVNEXT_LAYERS, FLOOR, PIT_OUT_MBLOCKS, SOURCE_SHAPES, SSL_OUT_MBLOCKS, WIDE_SHAPES_256, _bump_trips, _gate_case, convnext_prefixes,
                     gate_windows_and_rows, gemm_s2_width, ln_bound, oracle_one_thread, planted_errors_trip, rel_rms, rescaled_ln, row_errors,
                     sourcenet_edge_inputs, state_dicts, wide_tile_shapes, window_errors)
from oracle import ref_cpu as R
from tinyvc_amd import synth

ELU_TAIL = {(1, 1): ["amps row 14 x (1 + 1e-4)"]}          # see the module docstring


def _source(sd, inputs):
    return dict(zip(("amps", "kernel"), R.source_net(sd, *inputs)))


# ------------------------------------------------------------------------------------------------ metric and inputs
def test_row_errors_are_in_the_utterances_units():
    truth = torch.ones(2, 4, 10, dtype=torch.float64)
    truth[1] *= 1e3
    truth[:, 3] *= 1e-3                                      # a row far below the utterance's level
    rms0 = float(truth[0].pow(2).mean().sqrt())
    x = truth.clone()
    x[:, 1, :5] += 0.5
    e = row_errors(x, truth)
    assert e.shape == (2, 4) and float(e[:, [0, 2, 3]].max()) == 0.0
    assert abs(float(e[0, 1]) - 0.5 * 0.5 ** 0.5 / rms0) < 1e-12 and abs(float(e[1, 1]) - 0.5e-3 * 0.5 ** 0.5 / rms0) < 1e-12
    assert torch.equal(e, window_errors(x.transpose(1, 2), truth.transpose(1, 2), width=1))
    x = truth.clone()
    x[:, 3] *= 1.0 + 1e-4
    e = row_errors(x, truth)
    assert float(e[:, :3].max()) == 0.0
    assert abs(float(e[0, 3]) - 1e-7 / rms0) < 1e-12, "1e-4 of a row at 1e-3 of the utterance's level reads 1e-7, not 1e-4"


def test_the_whole_tensor_gate_passes_a_wrong_last_kernel_row():
    """test_decoder_stages holds `kernel` to one relative rms of 2e-6: row 960 off by 1e-4 reads below it, and 2e-5 under the row gate."""
    inp = sourcenet_edge_inputs(1, 129)
    _e, dec_sd = state_dicts(0)
    truth = _source({k: v.double() for k, v in dec_sd.items()}, [x.double() for x in inp])["kernel"]
    x = truth.clone()
    x[:, 960] *= 1.0 + 1e-4
    assert rel_rms(x, truth) < 2e-6
    assert float(row_errors(x, truth)[:, 960].min()) > 5 * FLOOR


def test_sourcenet_inputs_reach_both_f0_branches_and_both_ends_of_a_frame():
    for B, T in SOURCE_SHAPES:
        content, f0, energy = sourcenet_edge_inputs(B, T)
        assert content.shape == (B, 768, T) and f0.shape == (B, 1, T) and energy.shape == (B, 1, 480 * T)
        assert bool((f0[..., -1] == -5.0).all()) and bool((f0[..., 0:T - 1:3] == 0.0).all())
        if T >= 3:
            assert bool((f0[..., 1:T - 1:3] >= 80.0).all())
        where = energy.view(B, T, 480).argmax(dim=2)
        assert bool((where[:, 0::2] == 0).all()) and bool((where[:, 1::2] == 479).all())
        assert torch.equal(sourcenet_edge_inputs(B, T)[2], energy), "the inputs are a function of the shape alone"


# ------------------------------------------------------------------------------------------------ SourceNet gates
@pytest.mark.parametrize("B,T", SOURCE_SHAPES)
def test_oracle_sourcenet_passes_its_gates_and_each_planted_error_trips_them(B, T):
    _e, dec_sd = state_dicts(0)
    inp = sourcenet_edge_inputs(B, T)
    truth = _source({k: v.double() for k, v in dec_sd.items()}, [x.double() for x in inp])
    with oracle_one_thread():
        ref = _source(dec_sd, inp)
    fails, gates = gate_windows_and_rows(f"oracle source_net B={B} T={T}", ref, truth, ref, log=False)
    assert not fails
    # the floor decides: the yardstick's worst window and worst row are below half of it (measured: windows 0.8e-7 .. 2.3e-7, rows 1.8e-7 .. 1.0e-6)
    assert all(g == FLOOR for g in gates.values()), gates
    again = _source(dec_sd, inp)                              # on all threads: the same gates
    assert not gate_windows_and_rows("", again, truth, ref, log=False)[0]
    missed = planted_errors_trip(ref, truth, gates)
    assert missed == ELU_TAIL.get((B, T), []), missed
    if (B, T) in ELU_TAIL:
        a = truth["amps"]
        share = float(a[0, 14].pow(2).mean().sqrt() / a[0].pow(2).mean().sqrt())
        bumped = ref["amps"].double().clone()
        bumped[:, 14] *= 1.0 + 1e-4
        assert share < 0.01 and abs(float(row_errors(bumped, a)[0, 14]) - 1e-4 * share) < 1e-7 and 1e-4 * share < FLOOR


# ------------------------------------------------------------------------------------------------ encoder at the wide tiles
@pytest.mark.parametrize("B,T", WIDE_SHAPES_256)
def test_oracle_encoder_passes_its_window_gate_at_the_wide_shapes_and_a_two_column_error_trips_it(B, T):
    enc_sd, _d = state_dicts(0)
    e64 = {k: v.double() for k, v in enc_sd.items()}
    spec = R.spectrogram(synth.synth_wave(B, 480 * T, seed=2000 + T))
    truth = {"ssl": R.ssl_features(e64, spec.double()), "logits": R.pitch_logits(e64, spec.double())}
    with oracle_one_thread():
        ref = {"ssl": R.ssl_features(enc_sd, spec), "logits": R.pitch_logits(enc_sd, spec)}
    fails, gates = _gate_case(f"oracle encoder B={B} T={T}", ref, truth, ref)
    assert not fails
    assert all(bool((g == FLOOR).all()) for g in gates.values()), "the floor decides (measured: ssl 6.6e-7 .. 8.1e-7, logits 4.1e-8 .. 3.0e-7)"
    assert _bump_trips(ref, truth, gates, "ssl") and _bump_trips(ref, truth, gates, "logits")


def test_width_rule_at_256_cus():
    cols = [B * T for B, T in WIDE_SHAPES_256]
    assert cols == [2691, 4097, 5442, 6722]
    assert [gemm_s2_width(n, SSL_OUT_MBLOCKS, 256) for n in cols] == [3, 4, 5, 6]
    assert [gemm_s2_width(n, PIT_OUT_MBLOCKS, 256) for n in cols] == [2, 3, 3, 4]
    assert [n % (32 * w) for n, w in zip(cols, (3, 4, 5, 6))] == [3, 1, 2, 2]
    assert wide_tile_shapes(256) == WIDE_SHAPES_256
    # the ranges each width holds for ssl_out (6 m-blocks) and the first columns at which pit_out (4 m-blocks) leaves a width
    for w, (lo, hi) in {3: (2689, 4032), 4: (4033, 5376), 5: (5377, 6720), 6: (6721, 8064)}.items():
        assert {gemm_s2_width(n, SSL_OUT_MBLOCKS, 256) for n in (lo, (lo + hi) // 2, hi)} == {w}
    assert [gemm_s2_width(n, PIT_OUT_MBLOCKS, 256) for n in (4096, 4097, 6144, 6145)] == [2, 3, 3, 4]
    # every shape of test_encoder_per_window_at_tile_edges stays on the 64-column tile: the gap this file's GPU twin closes
    assert {gemm_s2_width(n, m, 256) for n in (96, 99, 192, 195, 1024, 1025) for m in (SSL_OUT_MBLOCKS, PIT_OUT_MBLOCKS)} == {2}
    # another chip: the picked shapes keep the properties, or the entry is None (the GPU test then skips with the reason)
    for ncu in (64, 240, 304):
        for want, s in zip((3, 4, 5, 6), wide_tile_shapes(ncu)):
            assert s is None or (gemm_s2_width(s[0] * s[1], SSL_OUT_MBLOCKS, ncu) == want and 1 <= s[0] * s[1] % (32 * want) <= 3)


# ------------------------------------------------------------------------------------------------ rescaled checkpoints
VARIANTS = {"A": "all", "B": "second"}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rescaled_checkpoints_are_the_same_function_and_leave_the_fused_path(variant):
    enc_sd, dec_sd = state_dicts(0)
    for sd, trunks in ((enc_sd, ("ssl_feature_estimator", "pitch_estimator")), (dec_sd, ("source_net",))):
        chosen = convnext_prefixes(trunks, VARIANTS[variant])
        res = rescaled_ln(sd, chosen)
        assert set(res) == set(sd) and {k for k in sd if not torch.equal(sd[k], res[k])} == {p + s for p in chosen for s in (".norm.gamma", ".norm.beta", ".c2.weight")}
        for p in convnext_prefixes(trunks):
            assert ln_bound(sd, p) < 32.0, (p, ln_bound(sd, p))                       # 14 .. 26 in the synthetic checkpoints: always fused
            assert (ln_bound(res, p) >= 32768.0) == (p in chosen), (p, ln_bound(res, p))
            if p in chosen:
                assert abs(ln_bound(res, p) - 4096.0 * ln_bound(sd, p)) < 1.0
    assert len(convnext_prefixes(CONVNEXT_LAYERS)) == 13 and len(convnext_prefixes(CONVNEXT_LAYERS, "second")) == 6
    assert "source_net.mid_layers.2" not in convnext_prefixes(("source_net",), "second"), "variant B: SourceNet's last layer stays fused"
    # the oracle's fp32 SourceNet and encoder outputs do not change by one bit
    res = rescaled_ln(dec_sd, convnext_prefixes(("source_net",), VARIANTS[variant]))
    inp = sourcenet_edge_inputs(3, 33)
    with oracle_one_thread():
        a, b = _source(dec_sd, inp), _source(res, inp)
    assert torch.equal(a["amps"], b["amps"]) and torch.equal(a["kernel"], b["kernel"])
    res = rescaled_ln(enc_sd, convnext_prefixes(("ssl_feature_estimator", "pitch_estimator"), VARIANTS[variant]))
    spec = R.spectrogram(synth.synth_wave(3, 480 * 33, seed=2033))
    with oracle_one_thread():
        assert torch.equal(R.ssl_features(enc_sd, spec), R.ssl_features(res, spec)) and torch.equal(R.pitch_logits(enc_sd, spec), R.pitch_logits(res, spec))
