"""The small kernels at both ends of the chain - |STFT|, energy envelope, pitch decode, oscillator and filtered noise - per frame, per bin,
per column and per sample, at the shortest lengths and at every store path.

test_front_end and test_decoder_stages hold these kernels to one whole-tensor relative rms at T = 28 and T = 50; bin 960 of every frame off by
1e-4 reads 1.3e-6 there and passes (tests/test_front_dsp_metric_host.py, which proves every gate and input below with the oracle alone).
Here the rule of test_gpu_tile_edges.py applies to single frames, bins and samples: the truth is the oracle evaluated in fp64, the yardstick
the oracle's own fp32 evaluation on one thread, and

    e_gpu <= max(floor, 2 x the worst e_ref of that case and metric)

1. Engine.stft_mag (stft_fft_kernel).  Per frame: rms over bins of x - truth over the rms of the whole row.  Per bin: rms over frames over
   the rms over frames of the truth at that bin.  No floor.  The oracle's worst frame is 1.3e-7 .. 1.9e-7; its worst bin 1.1e-6 .. 5.7e-6 on
   synth_wave and 2.6e-7 .. 1.5e-6 on the white spike signal (the fewer frames, the larger; the figures depend on the host's FFT: at
   (1, 3) synth_wave one host gives 7.4e-6 at bin 465, another 3.75e-6 at bin 150).  Bin 960 x (1 + 1e-4) and the last frame x (1 + 1e-5),
   applied to the GPU result on the host, must trip the gates.
   One case has a per-bin factor of 4 instead of 2 (helpers.STFT_BIN_FACTOR): (1, 3) synth_wave.  Measured: GPU 8.38e-6 at bin 225 against
   the oracle's 3.75e-6 at bin 150, a ratio of 2.23.  It is arithmetic spread, not a defect: only 240 of that input's 1440 samples are not
   silent, so its three frames are one short burst whose spectrum has deep valleys, and the per-bin figure divides a transform's roundoff -
   which scales with the frame, not with the bin - by the bin's own scale.  Bin 225 stands at 0.034 of the row's rms, the smallest scale of
   any case's worst bin; in the row's units its GPU error is 2.8e-7, against 4e-7 .. 5.7e-7 at the worst bins of the longer synth_wave
   cases (which pass at factor 2) and an oracle whose own per-bin errors reach 1e-6 of the row's rms on this input.  The worst bin of each
   implementation is another one (225 | 150 | 465), the case's per-frame figures are below the oracle's (1.46e-7 against 1.59e-7), bin 960
   and the reflecting frames show nothing, and the spike signal at the same shape passes at factor 2 (1.67e-6 against 1.46e-6, both at
   bin 207).  With three frames the maximum over 961 such ratios is heavy-tailed; 4 x 3.75e-6 = 1.5e-5 still trips on bin 960 x (1 + 1e-4).
2. Engine.energy (energy_pool_kernel + lerp_resize_kernel) against the FP32 oracle, element by element: the kernels restate ATen's fp32
   position arithmetic on purpose (the fp32 oracle is itself 2.3e-5 from fp64 at L = 61 920).  The pooled maxima are exact; with the same
   fp32 weights two evaluation orders of w0 a + w1 b differ by at most 1.5 ulp of the larger term: |gpu - ref| <= 2^-22 max|wav| of the row.
3. Engine.pitch_decode (pitch_decode_kernel) on logits of the test's own making, against helpers.decode_lower_id_first in fp64 (the oracle's
   torch.topk does not break ties towards the lower class: an all-equal column gives it classes [1, 3, 0, 2]).  Per element
   |gpu - truth| <= max(16 x 2^-24, 2 x the oracle's worst fp32 element) x truth - 16 roundings bound the sum of four positive products
   e_i / den f_i; the oracle's fp32 worst on the tie-free columns is 4.0e-7 (a column whose best class is 511), so the floor decides - and
   exactly 0 where the truth is 0.  No column's fp64 value lies within 1e-3 Hz of the 20 Hz gate (asserted).
4. Engine.dsp at T = 1 .. 17.  Noise row (noise_ifft_kernel, noise_ola_kernel) against R.oscillate_noise in fp64, per 480-sample frame and
   per element, both relative to the row's rms; the oracle's frames are 1.3e-7 .. 2.0e-7 and its elements up to 7.7e-7, also with the phases
   x 40 (the sincosf branch of the kernel).  A NaN phase makes exactly the oracle's NaN samples NaN.  1e-5 x rms on the first frame must trip
   the gates.  Harmonic rows (harm_* kernels) against the FP32 oracle - the fp64 one is another function: the phase is rounded to fp32 per
   sample by design - under the decidable-sample rule of test_gpu_long.py (helpers.decidable_samples) with the margin
   4 (i + 1) 2^-53 P_i, and every sample decidable where no fp64 addition of the row's increments can round at all
   (helpers.sums_exact_in_any_order: at these lengths a constant f0 puts P_i = (i + 1) c exactly ON fp32 rounding midpoints for a few per
   cent of the samples, and both sides round the tie to even).  Decidable samples hold |gpu - ref| <= 2^-21 |interpolated amp|; the others
   are at most 1e-3 of a case.
5. stft_fft_kernel's 16-byte store under a ragged batch's arbitrary first column (sbase = pre[b]) is already covered:
   test_gpu_index_build.py::test_ragged_encode_equals_one_call_per_utterance_and_the_oracle packs 3, 10, 11, 42, 43, 64, 65, 130 frames
   (368 columns, a multiple of 4) in one batch - the 11-frame utterance starts at column 13, the 42-frame one at column 24 - and holds every
   row's ssl and f0 to its own B = 1 stft_mag + encoder bit for bit.

Each case prints one `[front]` line: the worst GPU figure, the worst oracle figure and where it sits (profiles/front_dsp_edges.txt)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import (DECODE_SHAPES, DECODE_SPECIALS, DSP_SHAPES, ENERGY_LENGTHS, F0_PATTERNS, STFT_BIN_FACTOR, STFT_SHAPES, decidable_short, decode_edge_logits,
                     decode_lower_id_first, dsp_edge_f0, dsp_edge_inputs, energy_edge_wave, frame_bin_errors, frame_element_errors, harmonic_increments,
                     oracle_one_thread, state_dicts, stft_edge_wave)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV).encoder.engine(DEV)


def _where(e):
    """(row, column) of the largest entry of a [rows, n] tensor"""
    return divmod(int(e.argmax()), e.shape[1])


# ------------------------------------------------------------------------------------------------ 1. |STFT|
@pytest.mark.parametrize("kind", ["synth", "spikes"])
@pytest.mark.parametrize("B,T", STFT_SHAPES)
def test_stft_mag_per_frame_and_per_bin(eng, B, T, kind):
    """(B, T): (1, 3) L = 1440, the shortest legal input - every frame reflects at one end or both; (2, 4) a row stride that is a multiple of 4
    but less than one 8-frame group: the scalar store; (1, 7) less than one group; (2, 8) one full group on the float4 path, the second
    utterance at 961 x 8; (3, 9) odd row stride, a tail of one frame, all scalar; (2, 12) a float4 group and a scalar tail of 4 in one
    utterance; (1, 17) two groups and a tail of one frame."""
    wf = stft_edge_wave(kind, B, T)
    truth = R.spectrogram(wf.double())
    with oracle_one_thread():
        ref = R.spectrogram(wf)
    gpu = eng.stft_mag(wf.to(DEV)).cpu()
    assert gpu.shape == (B, 961, T) and torch.isfinite(gpu).all()
    fr_g, bin_g = frame_bin_errors(gpu, truth)
    fr_r, bin_r = frame_bin_errors(ref, truth)
    g_fr, g_bin = 2.0 * float(fr_r.max()), STFT_BIN_FACTOR.get((B, T, kind), 2.0) * float(bin_r.max())
    (rf, tf), (rb, kb) = _where(fr_g), _where(bin_g)
    own = float(torch.sqrt((truth[rb, kb] ** 2).mean() / (truth[rb] ** 2).mean()))      # the worst bin's own scale, in units of the row's rms
    print(f"[front] stft_mag B={B} T={T} {kind}: worst frame GPU {float(fr_g.max()):.2e} (row {rf} frame {tf}) / oracle {float(fr_r.max()):.2e} "
          f"(frame {_where(fr_r)[1]}); worst bin GPU {float(bin_g.max()):.2e} (row {rb} bin {kb}, its own scale {own:.3f} of the row's: {float(bin_g.max()) * own:.2e} of the row's rms) / oracle {float(bin_r.max()):.2e} (bin {_where(bin_r)[1]}); "
          f"bin 960 GPU {float(bin_g[:, 960].max()):.2e} / oracle {float(bin_r[:, 960].max()):.2e}")
    fails = [f"row {r} frame {t}: {float(fr_g[r, t]):.2e} > gate {g_fr:.2e}" for r, t in (fr_g > g_fr).nonzero().tolist()[:4]]
    fails += [f"row {r} bin {k}: {float(bin_g[r, k]):.2e} > gate {g_bin:.2e}" for r, k in (bin_g > g_bin).nonzero().tolist()[:4]]
    assert not fails, f"B={B} T={T} {kind}: " + "; ".join(fails)
    x = gpu.clone()
    x[:, 960] *= 1.0 + 1e-4
    assert float(frame_bin_errors(x, truth)[1].max()) > g_bin, "bin 960 off by 1e-4 must trip the per-bin gate"
    x = gpu.clone()
    x[:, :, -1] *= 1.0 + 1e-5
    assert float(frame_bin_errors(x, truth)[0].max()) > g_fr, "the last frame off by 1e-5 must trip the per-frame gate"


# ------------------------------------------------------------------------------------------------ 2. energy
@pytest.mark.parametrize("L", ENERGY_LENGTHS)
def test_energy_element_by_element(eng, L):
    """B = 1 and B = 3 at each length.  128: two pooled values, the shortest legal input; 129, 191 / 192 / 193: both sides of the third pooled
    value; 1437 .. 1440: n_out & 3 = 1, 2, 3, 0 - with B = 3 the odd ones are lerp_resize_kernel's scalar stores on unaligned rows -; 61 920 /
    61 921: several workgroups per row and, at 61 921, a length that is no whole number of frames (Engine.energy sizes its workspace from L
    rounded down to one)."""
    for B in (1, 3):
        wf = energy_edge_wave(B, L)
        with oracle_one_thread():
            ref = R.estimate_energy(wf)
        gpu = eng.energy(wf.to(DEV)).cpu()
        assert gpu.shape == (B, 1, L) and torch.isfinite(gpu).all()
        bound = 2.0 ** -22 * wf.abs().amax(dim=1).double()
        d = (gpu.double() - ref.double()).abs()[:, 0] / bound[:, None]
        r, i = _where(d)
        print(f"[front] energy B={B} L={L}: worst |gpu - oracle fp32| = {float(d.max()):.3f} x the bound 2^-22 max|wav| (row {r} sample {i}); "
              f"{int((d > 0).sum())} of {B * L} elements differ")
        assert float(d.max()) <= 1.0, f"B={B} L={L}: row {r} sample {i}: {float(d.max()):.3f} x the bound"


# ------------------------------------------------------------------------------------------------ 3. pitch decode
@pytest.mark.parametrize("B,T", DECODE_SHAPES)
def test_pitch_decode_on_constructed_logits(eng, B, T):
    """B T = 1 (one call per constructed column), 63, 64 (one full workgroup), 65 and 129 = 3 x 43 (a last workgroup with one live lane).
    Columns: helpers.decode_edge_logits."""
    floor = 16 * 2.0 ** -24
    for rot in (range(len(DECODE_SPECIALS)) if B * T == 1 else (0,)):
        lg, kinds = decode_edge_logits(B, T, rot)
        truth, raw, _ids, tie_free = decode_lower_id_first(lg.double())
        assert float((raw - 20.0).abs().min()) > 1e-3, "a column within 1e-3 Hz of the 20 Hz gate"
        with oracle_one_thread():
            ref = R.pitch_decode(lg)
        voiced = truth > 0
        m = tie_free[:, None, :] & voiced
        e_ref = float(((ref.double() - truth).abs() / truth)[m].max()) if m.any() else 0.0
        gate = max(floor, 2.0 * e_ref)
        gpu = eng.pitch_decode(lg.to(DEV)).cpu()
        assert gpu.shape == (B, 1, T)
        rel = torch.where(voiced, (gpu.double() - truth).abs() / truth.clamp_min(1e-300), torch.zeros_like(truth)).reshape(-1)
        n = int(rel.argmax())
        not_zero = (gpu[~voiced] != 0).reshape(-1)
        print(f"[front] pitch_decode B={B} T={T} rot={rot}: worst |gpu - truth| / truth {float(rel.max()):.2e} (column {n}, {kinds[n]}) / oracle fp32 on the "
              f"tie-free columns {e_ref:.2e}, gate {gate:.2e}; {int((~voiced).sum())} columns with truth 0, {int(not_zero.sum())} of them not exactly 0")
        bad = (rel > gate).nonzero().flatten().tolist()
        assert not bad, "; ".join(f"column {c} ({kinds[c]}): gpu {float(gpu.reshape(-1)[c])!r} truth {float(truth.reshape(-1)[c])!r}" for c in bad[:6])
        assert not not_zero.any(), "where the truth is 0 the output must be exactly 0: columns " + str([c for c in range(B * T) if not voiced.reshape(-1)[c] and gpu.reshape(-1)[c] != 0][:6])


# ------------------------------------------------------------------------------------------------ 4. dsp
def _noise_case(eng, B, T, angle, kern, amps, tag):
    """The noise row of one Engine.dsp call against the fp64 oracle -> failures.  NaN samples of the truth must be NaN, the others finite."""
    truth = R.oscillate_noise(kern.double(), angle.double())[:, 0]
    with oracle_one_thread():
        ref = R.oscillate_noise(kern, angle)[:, 0]
    f0 = dsp_edge_f0("unvoiced_first", B, T)
    gpu = eng.dsp(f0.to(DEV), amps.to(DEV), kern.to(DEV), noise_angle=angle.to(DEV)).cpu()
    assert gpu.shape == (B, 16, 480 * T)
    gpu = gpu[:, 15]
    nan = torch.isnan(truth)
    assert torch.equal(torch.isnan(ref), nan), "the two oracles disagree on the NaN samples"
    assert torch.equal(torch.isnan(gpu), nan), f"{tag}: NaN on {int(torch.isnan(gpu).sum())} samples, the oracle on {int(nan.sum())}"
    assert torch.isfinite(gpu[~nan]).all()
    fr_g, el_g = frame_element_errors(gpu, truth)
    fr_r, el_r = frame_element_errors(ref, truth)
    g_fr, g_el = 2.0 * float(fr_r.max()), 2.0 * float(el_r.max())
    (rf, tf), (re_, ie) = _where(fr_g), _where(el_g)
    print(f"[front] dsp noise row {tag}: worst frame GPU {float(fr_g.max()):.2e} (row {rf} frame {tf}) / oracle {float(fr_r.max()):.2e}; "
          f"worst element GPU {float(el_g.max()):.2e} (row {re_} sample {ie}) / oracle {float(el_r.max()):.2e}; NaN samples {int(nan.sum())}")
    fails = [f"row {r} frame {t}: {float(fr_g[r, t]):.2e} > gate {g_fr:.2e}" for r, t in (fr_g > g_fr).nonzero().tolist()[:4]]
    fails += [f"row {r} sample {i}: {float(el_g[r, i]):.2e} > gate {g_el:.2e}" for r, i in (el_g > g_el).nonzero().tolist()[:4]]
    x = torch.where(nan, torch.zeros_like(truth), gpu.double())
    x[:, :480] += 1e-5 * torch.sqrt((torch.where(nan, torch.zeros_like(truth), truth) ** 2).sum(dim=1) / (~nan).sum(dim=1))[:, None]
    x = torch.where(nan, truth, x)
    fr_b, el_b = frame_element_errors(x, truth)
    live = ~nan[:, :480]
    assert float(fr_b[:, 0][live.any(dim=1)].min()) > g_fr and float(el_b[:, :480][live].min()) > g_el, "1e-5 x rms on the first frame must trip both gates"
    return fails


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("B,T", DSP_SHAPES)
def test_noise_row_per_frame_and_per_element(eng, B, T, scale):
    """T = 1 and T = 2 are the lengths at which the overlap-add envelope counts the zero frame 0 for every sample; scale 40 sends the phases
    far outside [-2 pi, 2 pi], the kernel's sincosf branch."""
    amps, kern, angle = dsp_edge_inputs(B, T)
    fails = _noise_case(eng, B, T, angle * scale, kern, amps, f"B={B} T={T} phases x {scale:g}")
    assert not fails, f"B={B} T={T} x {scale:g}: " + "; ".join(fails)


def test_noise_row_with_a_nan_phase(eng):
    """One NaN phase at (row 1, bin 100, frame 4) of B = 2, T = 9: NaN exactly on the 1920 samples its frame covers, the gates elsewhere."""
    B, T = 2, 9
    amps, kern, angle = dsp_edge_inputs(B, T)
    angle[1, 100, 4] = float("nan")
    fails = _noise_case(eng, B, T, angle, kern, amps, f"B={B} T={T} NaN phase at (1, 100, 4)")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("B,T", DSP_SHAPES)
def test_harmonic_rows_on_decidable_samples(eng, B, T):
    """Every f0 pattern of helpers.F0_PATTERNS: voiced / unvoiced changes at frame 0 and at the last frame, exactly 20.0 (unvoiced) and the
    next float (voiced) on every other frame, all zero, 800 Hz.  At T = 1 .. 3 the oscillator's workgroup of four frames is mostly empty."""
    amps, kern, angle = dsp_edge_inputs(B, T)
    L = 480 * T
    with oracle_one_thread():
        amp_i = F.interpolate(amps, scale_factor=R.HOP, mode="linear")
    worst, at, nondec_worst, mismatched, exact_rows = 0.0, None, 0, 0, 0
    for pattern in F0_PATTERNS:
        f0 = dsp_edge_f0(pattern, B, T)
        with oracle_one_thread():
            ref = R.oscillate_harmonics(f0) * amp_i
        inc = harmonic_increments(f0)
        gpu = eng.dsp(f0.to(DEV), amps.to(DEV), kern.to(DEV), noise_angle=angle.to(DEV)).cpu()[:, :15]
        assert gpu.shape == (B, 15, L) and torch.isfinite(gpu).all()
        nondec = 0
        for b in range(B):
            for m in range(15):
                dec, _P, I = decidable_short(inc[b, m].numpy())
                if m in (0, 14):                                   # the model of the oracle's cumsum: fp64 sequential, rounded once
                    assert np.array_equal(torch.cumsum(inc[b:b + 1, m:m + 1], dim=2).reshape(-1).numpy(), I)
                amp = amp_i[b, m].numpy()
                diff = np.abs(gpu[b, m].numpy().astype(np.float64) - ref[b, m].numpy().astype(np.float64))
                bad = diff > 2.0 ** -21 * np.abs(amp) + 1e-30
                first = int(np.argmax(bad & dec))
                assert not (bad & dec).any(), (
                    f"B={B} T={T} {pattern}: row {b} harmonic {m + 1}: {int((bad & dec).sum())} decidable samples differ from the oracle, first at "
                    f"{first} (|diff| there {diff[first]:.3e}, 2^-21 |amp| there {2.0 ** -21 * abs(float(amp[first])):.3e})")
                nondec += int((~dec).sum())
                mismatched += int(bad.sum())
                exact_rows += int(dec.all())
                rel = diff[dec] / np.maximum(np.abs(amp[dec]), 1e-30)
                if rel.size and float(rel.max()) > worst:
                    worst, at = float(rel.max()), (pattern, b, m + 1, int(np.flatnonzero(dec)[int(rel.argmax())]))
        assert nondec <= 1e-3 * B * 15 * L, f"B={B} T={T} {pattern}: {nondec} non-decidable samples"
        nondec_worst = max(nondec_worst, nondec)
    print(f"[front] dsp harmonics B={B} T={T}, {len(F0_PATTERNS)} f0 patterns: worst decidable |gpu - oracle fp32| / |amp| {worst:.2e} = {worst * 2 ** 21:.3f} x the bound 2^-21 "
          f"at (pattern, row, harmonic, sample) {at}; at most {nondec_worst} of {B * 15 * L} samples of a pattern non-decidable (cap {1e-3 * B * 15 * L:.0f}), "
          f"{mismatched} samples outside the bound; {exact_rows} of {len(F0_PATTERNS) * B * 15} rows decidable throughout")
