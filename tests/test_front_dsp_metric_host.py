"""The gates and the inputs of test_gpu_front_dsp_edges.py, proved with the oracle alone (no GPU).

What the whole-tensor gate of test_front_end lets through, that the oracle's own fp32 evaluation passes every per-frame / per-bin / per-element
gate while a single wrong bin or frame trips it, that the restated pitch decode (helpers.decode_lower_id_first: ties go to the lower class id)
IS the oracle's decode wherever there is no tie, that no constructed decode column sits at the 20 Hz output gate, and that the oscillator's
non-decidable samples stay below the cap of 1e-3 of a case at every f0 pattern."""
import numpy as np
import pytest
import torch

from helpers import (DECODE_SHAPES, DECODE_SPECIALS, DSP_SHAPES, F0_PATTERNS, STFT_BIN_FACTOR, STFT_SHAPES, decidable_short, decode_edge_logits, decode_lower_id_first,
                     dsp_edge_f0, dsp_edge_inputs, frame_bin_errors, frame_element_errors, harmonic_increments, oracle_one_thread, rel_rms, stft_edge_wave)
from oracle import ref_cpu as R
from tinyvc_amd import synth


# ------------------------------------------------------------------------------------------------ |STFT|
def test_the_whole_tensor_gate_passes_a_wrong_nyquist_bin():
    """test_front_end's gate is one relative rms of 1.5e-6 over [B, 961, T].  Bin 960 of every frame off by 1e-4 reads about 1.3e-6 there
    (T = 28 and T = 50) and passes; relative to the bin's own scale it reads 1e-4."""
    for T in (28, 50):
        truth = R.spectrogram(synth.synth_wave(2, 480 * T, seed=100).double())
        x = truth.clone()
        x[:, 960] *= 1.0 + 1e-4
        assert rel_rms(x, truth) < 1.5e-6
        _fr, bins = frame_bin_errors(x, truth)
        assert abs(float(bins[:, 960].min()) - 1e-4) < 1e-9 and float(bins[:, :960].max()) == 0.0


@pytest.mark.parametrize("kind", ["synth", "spikes"])
@pytest.mark.parametrize("B,T", STFT_SHAPES)
def test_oracle_spectrogram_passes_its_gates_and_one_wrong_bin_or_frame_trips_them(B, T, kind):
    wf = stft_edge_wave(kind, B, T)
    truth = R.spectrogram(wf.double())
    with oracle_one_thread():
        ref = R.spectrogram(wf)
    fr, bins = frame_bin_errors(ref, truth)
    g_fr, g_bin = 2.0 * float(fr.max()), STFT_BIN_FACTOR.get((B, T, kind), 2.0) * float(bins.max())
    # the oracle's own figures: what the factor 2 stands on (the module docstring of test_gpu_front_dsp_edges.py quotes these ranges)
    assert 5e-8 < float(fr.max()) < 3e-7 and 1e-7 < float(bins.max()) < 1.2e-5, (float(fr.max()), float(bins.max()))
    again = R.spectrogram(wf)                                  # on all threads: the same gates
    fr2, bins2 = frame_bin_errors(again, truth)
    assert float(fr2.max()) <= g_fr and float(bins2.max()) <= g_bin
    x = ref.clone()
    x[:, 960] *= 1.0 + 1e-4
    assert float(frame_bin_errors(x, truth)[1].max()) > g_bin, "bin 960 off by 1e-4 must trip the per-bin gate"
    x = ref.clone()
    x[:, :, -1] *= 1.0 + 1e-5
    assert float(frame_bin_errors(x, truth)[0].max()) > g_fr, "the last frame off by 1e-5 must trip the per-frame gate"


def test_the_spike_signal_shows_a_reflection_off_by_one():
    """Reflecting about sample -1 / L instead of 0 / L - 1 (x[-n] = x[n - 1]) changes frames 0, T - 2 and T - 1 of the spike signal by far
    more than any gate, and no other frame."""
    B, T = 1, 7
    wf = stft_edge_wave("spikes", B, T).double()
    truth = R.spectrogram(wf)
    pad = torch.cat([wf[:, :960].flip(1), wf, wf[:, -960:].flip(1)], dim=1)          # symmetric padding: off by one at both ends
    win = torch.hann_window(1920, dtype=torch.float64)
    wrong = torch.stft(pad, 1920, 480, window=win, center=False, return_complex=True).abs()[:, :, 1:]
    fr, _bins = frame_bin_errors(wrong, truth)
    assert float(fr[0, [0, T - 2, T - 1]].min()) > 1e-3 and float(fr[0, 1:T - 2].max()) < 1e-12


# ------------------------------------------------------------------------------------------------ pitch decode
def _all_decode_cases():
    for B, T in DECODE_SHAPES:
        for rot in (range(len(DECODE_SPECIALS)) if B * T == 1 else (0,)):
            yield B, T, rot


def test_restated_decode_is_the_oracles_where_there_is_no_tie():
    seen = 0
    for B, T, rot in _all_decode_cases():
        lg, _kinds = decode_edge_logits(B, T, rot)
        f0, _raw, ids, tie_free = decode_lower_id_first(lg.double())
        want = R.pitch_decode(lg.double())
        m = tie_free[:, None, :]
        assert torch.equal(f0[m], want[m]), "the restatement differs from the oracle on tie-free logits"
        # the class lists too: the oracle's topk returns the same four classes in the same order there
        oids = torch.topk(lg.double(), 4, dim=1).indices
        assert torch.equal(ids.transpose(1, 2)[tie_free], oids.transpose(1, 2)[tie_free])
        seen += int(tie_free.sum())
    assert seen > 150


def test_restated_decode_sends_ties_to_the_lower_class():
    cases = {"all_equal": [0, 1, 2, 3], "tie_top_31_32": [31, 32, 100, 200], "tie_top_5_500": [5, 500, 250, 251], "tie_4th_31_32": [100, 200, 300, 31],
             "tie_4th_5_500": [150, 160, 170, 5], "tie_4th_three_way": [10, 20, 30, 63], "four_waves": [10, 170, 300, 511], "two_finite_tied": [7, 480, 0, 1]}
    lg, kinds = decode_edge_logits(3, 43)
    _f0, _raw, ids, tie_free = decode_lower_id_first(lg.double())
    ids = ids.transpose(1, 2).reshape(-1, 4)
    for kind, want in cases.items():
        n = kinds.index(kind)
        assert ids[n].tolist() == want, (kind, ids[n].tolist())
    assert not tie_free.reshape(-1)[kinds.index("tie_4th_31_32")] and tie_free.reshape(-1)[kinds.index("four_waves")]
    # torch.topk does not: the reason the oracle cannot be the reference on ties
    assert torch.topk(torch.ones(1, 512, 1), 4, dim=1).indices.flatten().tolist() != [0, 1, 2, 3]


def test_no_decode_column_sits_at_the_output_gate_and_the_oracle_fp32_error_is_small():
    worst = 0.0
    kinds_seen = set()
    for B, T, rot in _all_decode_cases():
        lg, kinds = decode_edge_logits(B, T, rot)
        kinds_seen |= set(kinds)
        f0, raw, _ids, tie_free = decode_lower_id_first(lg.double())
        assert float((raw - 20.0).abs().min()) > 1e-3, "a column within 1e-3 Hz of the 20 Hz gate: fp32 may land on the other side"
        with oracle_one_thread():
            ref = R.pitch_decode(lg)
        m = tie_free[:, None, :] & (f0 > 0)
        assert torch.equal(ref[tie_free[:, None, :] & (f0 == 0)].double(), f0[tie_free[:, None, :] & (f0 == 0)])
        if m.any():
            worst = max(worst, float(((ref.double() - f0).abs() / f0)[m].max()))
    assert kinds_seen == set(DECODE_SPECIALS) | {"prior", "prior_class0"}
    assert worst < 8 * 2.0 ** -24, worst          # 2 x this is below the 16 x 2^-24 floor: the floor decides the gate


# ------------------------------------------------------------------------------------------------ noise row
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("B,T", DSP_SHAPES)
def test_oracle_noise_row_passes_its_gates_and_a_wrong_first_frame_trips_them(B, T, scale):
    _amps, kern, angle = dsp_edge_inputs(B, T)
    angle = angle * scale
    truth = R.oscillate_noise(kern.double(), angle.double())[:, 0]
    with oracle_one_thread():
        ref = R.oscillate_noise(kern, angle)[:, 0]
    fr, el = frame_element_errors(ref, truth)
    assert 5e-8 < float(fr.max()) < 3e-7 and float(el.max()) < 1.2e-6, (float(fr.max()), float(el.max()))     # x 40: the oracle's error does not grow
    x = ref.double().clone()
    x[:, :480] += 1e-5 * torch.sqrt((truth * truth).mean(dim=1))[:, None]
    fr2, el2 = frame_element_errors(x, truth)
    assert float(fr2[:, 0].min()) > 2.0 * float(fr.max()) and float(el2[:, :480].min()) > 2.0 * float(el.max())


def test_a_nan_phase_makes_exactly_its_own_frame_nan_in_the_oracle():
    B, T = 2, 9
    _amps, kern, angle = dsp_edge_inputs(B, T)
    angle[1, 100, 4] = float("nan")
    truth = R.oscillate_noise(kern.double(), angle.double())[:, 0]
    ref = R.oscillate_noise(kern, angle)[:, 0]
    want = torch.zeros(B, 480 * T, dtype=torch.bool)
    want[1, 480 * 5 - 960:480 * 5 + 960] = True                 # frame 4 is frame 5 of the zero-prepended iSTFT: [2400, 4320) - 960
    assert torch.equal(torch.isnan(truth), want) and torch.equal(torch.isnan(ref), want)
    fr, el = frame_element_errors(ref, truth)
    assert torch.isfinite(fr).all() and torch.isfinite(el).all() and float(fr.max()) < 3e-7


# ------------------------------------------------------------------------------------------------ harmonic rows
@pytest.mark.parametrize("B,T", DSP_SHAPES)
def test_non_decidable_oscillator_samples_stay_below_the_cap(B, T):
    """Per case (shape, f0 pattern), all 15 rows: at most 1e-3 of the samples lie within 4 (i + 1) 2^-53 P_i of a rounding midpoint of the
    fp32 phase.  Also the model the rule stands on: ATen's cumsum of fp32 increments is the sequential fp64 sum, rounded once."""
    for pattern in F0_PATTERNS:
        f0 = dsp_edge_f0(pattern, B, T)
        inc = harmonic_increments(f0)
        nondec = 0
        for b in range(B):
            for m in range(15):
                dec, _P, I = decidable_short(inc[b, m].numpy())
                nondec += int((~dec).sum())
                if m in (0, 14):
                    assert np.array_equal(torch.cumsum(inc[b:b + 1, m:m + 1], dim=2).reshape(-1).numpy(), I)
        assert nondec <= 1e-3 * B * 15 * 480 * T, (pattern, nondec)
