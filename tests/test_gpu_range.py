"""The fp16 range guard of the split-precision kernels (split_fp16.h: block floating point).

Every fp32 operand is multiplied as two fp16 parts; fp16 tops out at 65 504 and loses relative precision below 6e-5, the fp32
reference does neither.  The guard: weights normalised per 32-row m-tile at pack time, activations scaled by a per-utterance power
of two taken from the tensor's |max| slot (written by the producing kernel) whenever that |max| is outside [2^-10, 2^15).  These
tests drive activations far outside fp16's range on both sides and require the same accuracy against the oracle as at O(1), and
that an out-of-range utterance leaves its batch mates untouched (the slots are per utterance)."""
import pytest
import torch

from helpers import load_golden, oracle_one_thread, rel_rms, state_dicts
from oracle import ref_cpu as R
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


@pytest.mark.parametrize("scale", [3e4, 1.0, 1e-7])
def test_encoder_on_out_of_range_spectrograms(gen, scale):
    """|STFT| of a waveform scaled by 3e4 peaks near 1e6 (> 65 504); scaled by 1e-7 it stays below 1e-5 (< 6e-5, fp16's smallest
    normal).  SSL features and pitch logits vs the oracle on the SAME spectrogram: the gates of the O(1) case."""
    from tinyvc_amd.module import utils
    enc_sd, _dec_sd = state_dicts(0)
    wf = synth.synth_wave(2, 9600 * 2, seed=31) * scale
    spec = utils.spectrogram(wf.to(DEV))
    with oracle_one_thread():
        ssl_ref = R.ssl_features(enc_sd, spec.cpu())
        log_ref = R.pitch_logits(enc_sd, spec.cpu())
    eng = gen.encoder.engine(DEV)
    ssl, _f0, logits = eng.encoder(spec, want_logits=True)
    print(f"[range] encoder, wave x {scale:g}: |spec| max {float(spec.abs().max()):.3g}; ssl rel {rel_rms(ssl.cpu(), ssl_ref):.2e}, "
          f"logits rel {rel_rms(logits.cpu(), log_ref):.2e}")
    assert torch.isfinite(ssl).all() and torch.isfinite(logits).all()
    assert rel_rms(ssl.cpu(), ssl_ref) <= 1e-5
    assert rel_rms(logits.cpu(), log_ref) <= 6e-6


@pytest.mark.parametrize("scale,T", [(1e5, 28), (1e-6, 28), (1e5, 140), (1.0, 140), (1e-6, 140)])
def test_filter_net_blocks_out_of_range(gen, scale, T):
    """FilterNet with `source` / `energy` scaled by 1e5 (every activation of the down path is far beyond 65 504) or 1e-6 (below
    fp16's normal range) and `content` by 1e3 / 1e-3: every Downsample / Upsample block output against the oracle on the same
    inputs, at the O(1) gate (3e-6; a block whose operands overflowed or flushed would be off by orders of magnitude).
    T = 140: every level is at least one 256-column tile long, so the 96 / 192 / 384-channel FiLM convs run on film_s2.h (single
    accumulators, operands normalised by their |max| slots); at T = 28 only the 96-channel level does."""
    _enc_sd, dec_sd = state_dicts(0)
    if T == 28:
        g = load_golden("convert_T28")
        content = torch.from_numpy(g["matched"])
        f0s = torch.from_numpy(g["f0s"])
    else:
        gi = torch.Generator().manual_seed(17)
        content = torch.randn(2, 768, T, generator=gi) * 0.5
        f0s = 80.0 + 200.0 * torch.rand(2, 1, T, generator=gi)
    content = content * (1e3 if scale > 1 else (1e-3 if scale < 1 else 1.0))
    B, _c, T = content.shape
    L = T * 480
    gsrc = torch.Generator().manual_seed(5)
    source = torch.randn(B, 16, L, generator=gsrc) * 0.3 * scale
    energy = torch.rand(B, 1, L, generator=gsrc) * scale
    with oracle_one_thread():
        _out, skips_ref, ups_ref = R.filter_net(dec_sd, content, f0s, energy, source, return_blocks=True)
    eng = gen.decoder.engine(DEV)
    wave, skips, ups = eng.filter_net(content.to(DEV), f0s.to(DEV), energy.to(DEV), source.to(DEV), blocks=True)
    assert torch.isfinite(wave).all()
    worst = 0.0
    for i, (s, r) in enumerate(zip(skips, skips_ref)):
        e = rel_rms(s.cpu(), r)
        worst = max(worst, e)
        print(f"[range] x{scale:g} downs[{i}] |max| {float(r.abs().max()):.3g} rel {e:.2e}")
        assert e <= 3e-6
    for i, (u, r) in enumerate(zip(ups, ups_ref[:4])):
        e = rel_rms(u.cpu(), r)
        worst = max(worst, e)
        print(f"[range] x{scale:g} ups[{i}] |max| {float(r.abs().max()):.3g} rel {e:.2e}")
        assert e <= 3e-6
    if scale > 1:
        assert max(float(r.abs().max()) for r in skips_ref) > 65504 and float(source.abs().max()) > 65504
    elif scale < 1:
        assert float(source.abs().max()) < 6e-5 and float(energy.abs().max()) < 6e-5      # (the biases bring the activations back to O(0.1))


def test_out_of_range_utterance_leaves_its_batch_mates_untouched(gen):
    """The |max| slots are per utterance: a batch whose first utterance is 1e5 times too loud (and whose second contains an Inf sample)
    converts the ordinary third utterance to exactly the samples it gets alone."""
    tgt = synth.synth_index(500, seed=3).to(DEV)
    wf = synth.synth_wave(3, 9600, seed=41)
    angle = synth.synth_angle(3, 20, 42).to(DEV)
    alone = gen.convert(wf[2:3].to(DEV), tgt, 0.0, noise_angle=angle[2:3])
    loud = wf.clone()
    loud[0] *= 1e5
    loud[1, 4000] = float("inf")
    out = gen.convert(loud.to(DEV), tgt, 0.0, noise_angle=angle)
    assert torch.equal(out[2:3], alone)
    assert torch.isfinite(out[0]).all(), "the loud utterance itself must convert (the reference does)"
    # and the loud utterance equals the reference on the same input to the usual relative accuracy of its waveform
    enc_sd, dec_sd = state_dicts(0)
    with oracle_one_thread():
        ref = R.convert(enc_sd, dec_sd, loud[:1], tgt.cpu(), 0.0, angle[:1].cpu())
    e = rel_rms(out[0].cpu(), ref[0])
    print(f"[range] utterance scaled by 1e5: waveform rel rms vs the oracle {e:.2e} (|wave| max {float(ref.abs().max()):.3g})")
    assert e <= 2e-3


@pytest.mark.parametrize("scale", [1e4, 1e-7, 1.0])
def test_ragged_rows_equal_their_own_calls_at_any_input_amplitude(gen, scale):
    """The whole-path call derives the |max| slots of |STFT| / energy from max |wav| per utterance (analytic bounds) - in a ragged batch exactly
    as in the equal-length call, so an utterance's power-of-two scales, and with them its bits, are those of its own B = 1 call even when the
    input is far outside fp16's window (un-normalised int16-range floats x 1e4; near silence x 1e-7)."""
    frames = [50, 9, 131, 20, 131]
    lens = [480 * f for f in frames]
    wf = torch.zeros(len(frames), max(lens))
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=70 + b)[0] * scale
    wf = wf.to(DEV)
    tgt = synth.synth_index(500, seed=8).to(DEV)
    angle = synth.synth_angle(len(frames), max(frames), 5).to(DEV)
    out = gen.convert(wf, tgt, 0.0, noise_angle=angle, lengths=lens)
    assert torch.isfinite(out).all()
    for b, f in enumerate(frames):
        one = gen.convert(wf[b:b + 1, :lens[b]], tgt, 0.0, noise_angle=angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b, :lens[b]], one[0]), f"scale {scale:g}, utterance {b} ({f} frames)"


def test_large_magnitude_index_is_range_guarded_through_the_blob_bound(gen):
    """The decoder takes the bound of the matched content from the prepared blob's header (the raw vectors' |max|).  An index whose vectors
    are 1e5 times larger (cosine matching does not care; the matched content is 1e5 times larger and far outside fp16) must convert like the
    oracle: a lost bound (0 = "no scaling") would overflow the fp16 parts of SourceNet's / FilterNet's first contraction to Inf."""
    from helpers import oracle_one_thread, state_dicts as sds
    from oracle import ref_cpu as R
    enc_sd, dec_sd = sds(0)
    wf = synth.synth_wave(1, 480 * 40, seed=17)
    tgt = synth.synth_index(700, seed=8) * 1e5
    angle = synth.synth_angle(1, 40, 3)
    out = gen.convert(wf.to(DEV), tgt.to(DEV), 0.0, noise_angle=angle.to(DEV)).cpu()
    assert torch.isfinite(out).all()
    # a content 1e5 times too large drives the decoder far out of its trained range (output rms ~ 5e12): the path is ill-conditioned there and
    # the reference's own fp32 arithmetic is 4e-3 (relative) away from the fp64 evaluation.  So both are measured against that truth
    # (test_gpu_truth.py's yardstick): the GPU may not be further from it than twice the reference's fp32 ops are.
    with oracle_one_thread():
        ref = R.convert(enc_sd, dec_sd, wf, tgt, 0.0, angle)
        truth = R.convert({k: v.double() for k, v in enc_sd.items()}, {k: v.double() for k, v in dec_sd.items()}, wf.double(), tgt.double(), 0.0, angle.double())
    nrm = (truth ** 2).mean().sqrt()
    e_gpu = float(((out.double() - truth) ** 2).mean().sqrt() / nrm)
    e_ref = float(((ref.double() - truth) ** 2).mean().sqrt() / nrm)
    print(f"[range] index x 1e5: rel rms vs the fp64 evaluation: GPU {e_gpu:.3e}, reference fp32 {e_ref:.3e}")
    assert e_gpu <= 2.0 * e_ref + 1e-6, (e_gpu, e_ref)


def test_foreign_blobs_are_checked_once_and_old_formats_refused(gen):
    """A prepared index at an address this process did not prepare (a clone) has its header read on first use: a faithful copy works and gives
    the same bits; a header with another format version, a wrong magic or another N is refused instead of silently running without the
    content bound (the |max| field was added without a version)."""
    from tinyvc_amd import _lib
    eng = gen.engine(DEV)
    tgt = synth.synth_index(600, seed=8).to(DEV)
    blob, n = eng.knn_prepare(tgt[0])
    src = synth.synth_tensor("q", (1, 768, 30), seed=4).to(DEV)
    ref = eng.knn_match(src, blob, n)
    copy = blob.clone()
    assert torch.equal(eng.knn_match(src, copy, n), ref)
    hdr = copy.view(torch.int32)
    assert int(hdr[5]) == 2 and int(hdr[2]) == 600
    for word, value, what in ((5, 1, "format version"), (0, 0x12345678, "not a blob"), (2, 601, "prepared for N")):
        bad = blob.clone()
        bad.view(torch.int32)[word] = value
        with pytest.raises(_lib.TinyVCError) as ei:
            eng.knn_match(src, bad, n)
        assert what in str(ei.value), str(ei.value)
