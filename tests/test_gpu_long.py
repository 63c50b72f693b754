"""Five-minute utterances (BASELINE configs[4]: T = 15 000 frames, L = 7.2 M samples) against the live oracle.

The other live comparisons stop at T = 1000.  At this length the oscillator's phase prefix reaches 1e6 cycles, where one fp32 ulp of it is
1/16 cycle: the harmonic kernels (decoder.hip: frame sums, frame scan, in-frame scan) add their fp64 sums in another order than the oracle's
sequential cumsum, so a sample is compared only where that order cannot flip the fp32 rounding of the prefix (the decidable samples, like the
kNN tests' near-tie mask).  Also the whole decoder on oracle inputs, and a ragged batch whose short utterances sit behind the long one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import decidable_samples, rel_rms, rms, state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 15000
L = T * R.HOP


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


def long_f0(B, seed):
    """[B, 1, T] f0 as pitch_decode emits it: voiced runs of 5 ... 400 frames between 20 and 800 Hz (a slow glide with vibrato), every
    eighth run just above the 20 Hz gate, and unvoiced runs of exactly 0 (about a third of the frames)."""
    g = np.random.default_rng(seed)
    f0 = np.zeros((B, 1, T), np.float32)
    just_above = np.nextafter(np.float32(20.0), np.float32(np.inf))
    for b in range(B):
        t, run = 0, 0
        while t < T:
            n = min(int(g.integers(5, 401)), T - t)
            if g.random() < 0.35:
                t += n                                                        # unvoiced: exact zeros
                continue
            if run % 8 == 7:
                v = just_above + np.float32(1e-3) * g.random(n).astype(np.float32)
            else:
                a, z = g.uniform(21.0, 800.0, 2)
                v = np.geomspace(a, z, n) * (1 + 0.01 * np.sin(np.arange(n) * g.uniform(0.1, 1.0)))
                v = np.clip(v, 20.01, 800.0).astype(np.float32)
            f0[b, 0, t:t + n] = v
            t += n
            run += 1
    return torch.from_numpy(f0)


def test_oscillator_and_noise_at_five_minutes_against_the_oracle():
    """tvc_dsp_f32 at B = 2, T = 15 000 against R.dsp on the same f0 / amps / kernel / phases.
    Harmonic rows 0-14: the oracle's phase is P = the sequential fp64 sum of its fp32 increments, rounded to fp32 (I).  Where P lies more
    than 1e-7 cycles from both rounding midpoints of I, any summation order within that drift gives the same I, hence the same sample up to
    the sine's last bit: |gpu - ref| <= 2^-21 |interpolated amp| there.  Samples outside that bound may only be non-decidable ones, at most
    64 over both utterances and all 15 rows.  Noise row 15: the 2e-6 relative gate of test_decoder_stages."""
    from tinyvc_amd.engine import default_engine
    eng = default_engine(torch.device(DEV))
    B = 2
    f0 = long_f0(B, 15)
    g = torch.Generator().manual_seed(16)
    amps = 0.05 + 2.0 * torch.rand(B, R.NUM_HARMONICS + 1, T, generator=g)
    kern = 0.05 + torch.rand(B, R.FFT_BIN, T, generator=g)
    angle = synth.synth_angle(B, T, 17)
    src = eng.dsp(f0.to(DEV), amps.to(DEV), kern.to(DEV), noise_angle=angle.to(DEV))
    assert src.shape == (B, 16, L)
    nondec = mismatched = 0
    worst_dec = 0.0
    for b in range(B):
        got = src[b].cpu()
        ref = R.dsp(f0[b:b + 1], amps[b:b + 1], kern[b:b + 1], angle[b:b + 1])[0]
        assert torch.isfinite(got).all()
        fs = F.interpolate(f0[b:b + 1], L, mode="linear")                      # the oracle's increments, op for op (oscillate_harmonics)
        amp_i = F.interpolate(amps[b:b + 1], scale_factor=R.HOP, mode="linear")[0]
        for m in range(R.NUM_HARMONICS + 1):
            inc = (fs * (m + 1)) / R.SAMPLE_RATE
            decidable, _P, I = decidable_samples(inc.reshape(-1).numpy(), 1e-7)
            if m in (0, R.NUM_HARMONICS):                                      # the model of the oracle's cumsum: fp64 sequential, rounded once
                assert np.array_equal(torch.cumsum(inc, dim=2).reshape(-1).numpy(), I)
            amp = amp_i[m].numpy()
            diff = np.abs(got[m].numpy().astype(np.float64) - ref[m].numpy().astype(np.float64))
            bad = diff > 2.0 ** -21 * np.abs(amp) + 1e-30
            assert not (bad & decidable).any(), (
                f"utterance {b}, harmonic {m + 1}: {int((bad & decidable).sum())} decidable samples differ from the oracle, first at "
                f"{int(np.argmax(bad & decidable))} (|diff| {diff[bad & decidable].max():.3e})")
            nondec += int((~decidable).sum())
            mismatched += int(bad.sum())
            worst_dec = max(worst_dec, float((diff[decidable] / np.maximum(np.abs(amp[decidable]), 1e-30)).max(initial=0.0)))
        noise = rel_rms(got[15], ref[15])
        print(f"[long] dsp utterance {b}: noise row rel rms {noise:.3e} (gate 2e-6)")
        assert noise <= 2e-6
        del got, ref, fs, amp_i
    print(f"[long] dsp T = {T}, B = {B}, 15 harmonic rows: {nondec} of {B * 15 * L} samples non-decidable at 1e-7 cycles, "
          f"{mismatched} outside 2^-21 |amp| (all non-decidable); worst decidable |diff| / |amp| {worst_dec:.3e}")
    assert mismatched <= 64


def test_decoder_at_five_minutes_on_oracle_inputs(gen):
    """The whole decoder (SourceNet, oscillator + noise, FilterNet) at T = 15 000 on synthetic content / f0 / energy, against
    R.decoder_infer run live: the 1e-5 rms gate of the 20 s decoder check in test_gpu_edges.py.  The stages are logged beside it."""
    enc_sd, dec_sd = state_dicts(0)
    g = torch.Generator().manual_seed(21)
    content = 0.5 * torch.randn(1, 768, T, generator=g)
    f0 = long_f0(1, 22)
    energy = R.estimate_energy(synth.synth_wave(1, L, seed=23))
    angle = synth.synth_angle(1, T, 24)
    with torch.inference_mode():                                             # R.decoder_infer, stage by stage
        amps, kern = R.source_net(dec_sd, content, f0, energy)
        src = R.dsp(f0, amps, kern, angle)
        ref = R.filter_net(dec_sd, content, f0, energy, src).squeeze(1)
    d_content, d_f0, d_energy, d_angle = content.to(DEV), f0.to(DEV), energy.to(DEV), angle.to(DEV)
    wave = gen.decoder.infer(d_content, d_f0, d_energy, noise_angle=d_angle)
    assert wave.shape == (1, L) and torch.isfinite(wave).all()
    d = rms(wave.cpu() - ref)
    _w, g_amps, g_kern, g_src = gen.engine(DEV).decoder(d_content, d_f0, d_energy, d_angle, stages=True)
    print(f"[long] 5-minute decoder (oracle inputs): rms diff {d:.3e} (gate 1e-5, as the 20 s check), wave rms {rms(ref):.3e}; stages rel rms: "
          f"amps {rel_rms(g_amps.cpu(), amps):.3e}, kernel {rel_rms(g_kern.cpu(), kern):.3e}, "
          f"harmonics {rel_rms(g_src[:, :15].cpu(), src[:, :15]):.3e}, noise {rel_rms(g_src[:, 15].cpu(), src[:, 15]):.3e}")
    assert d <= 1e-5


def test_ragged_batch_with_a_five_minute_utterance_in_front(gen):
    """tvc_convert_ragged_f32 with the 5-minute utterance first, so the short ones (61 frames, not padded to a frame; 200 frames) sit behind
    a 7.2 M-sample offset in every kernel: each row equals its own B = 1 call bit for bit, and the tails stay zero."""
    frames = [T, 61, 200]
    lens = [R.HOP * T, 61 * R.HOP - 17, 200 * R.HOP]
    wf = torch.zeros(3, L)
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=30 + b)[0]
    tgt = synth.synth_index(2000, seed=33).to(DEV)
    angle = synth.synth_angle(3, T, 34)
    out = gen.convert(wf.to(DEV), tgt, 0.5, noise_angle=angle.to(DEV), lengths=lens)
    assert out.shape == (3, L) and torch.isfinite(out).all()
    for b, f in enumerate(frames):
        n = R.HOP * f
        one = gen.convert(wf[b:b + 1, :lens[b]].to(DEV), tgt, 0.5, noise_angle=angle[b:b + 1, :, :f].contiguous().to(DEV))
        assert one.shape == (1, n)
        assert torch.equal(out[b, :n], one[0]), f"utterance {b} ({f} frames): ragged batch != its own B = 1 call"
        assert not out[b, n:].any(), "the tail of a row is zero-filled"
    print(f"[long] ragged batch of {frames} frames, the 5-minute utterance first: every row equals its B = 1 call bit for bit")
