"""FilterNet and encoder block outputs, window by window, at the lengths that put a tile tail or a kernel boundary on a seam.

Every FilterNet level picks its kernel or its column-tile width from the utterance's length (or, in one place, from the batch size), and so
does the encoder.  Such kernels go wrong in the last tile of an utterance - a halo replicate-padded past a short tail - and where another
instantiation takes over.  The block-wise comparisons elsewhere run at T = 28, 50, 140, 200 under a whole-tensor relative rms of 3e-6, which
an error of 1e-4 in the last two columns of a 3096-column block passes (2.5e-6: tests/test_window_metric_host.py).

Here every compared tensor is measured in 32-column windows (helpers.window_errors) against the truth, and so is the oracle's own fp32
evaluation on one thread, the yardstick.  The gate, for every tensor, row and window w:

    e_gpu(w) <= max(3e-6, 2 * max_w e_ref(w))

3e-6 is the block gate of test_filter_net_blocks, now per window; the factor 2 over the reference arithmetic's own error is the rule of the
phase-vocoder head and of the large-magnitude index (test_gpu_range.py).

The truth is the oracle evaluated in fp64 - EXCEPT the F.interpolate source positions (helpers.filter_edge_oracle, oracle.ref_cpu.fp32_positions):
src, i0 and lambda are the fp32 numbers ATen computes for fp32 tensors, src = fma(scale, dst + 0.5, -0.5), which the kernels restate on purpose
(small_kernels.h:lerp_coord); they are then used as fp64 weights.  On `.double()` tensors ATen takes the positions in fp64, and one ulp of the
fp32 `src` at column 48 000 is 2^-8 of a sample: against that plain fp64 truth (test_gpu_truth.py's, and this file's before) the oracle's own
worst waveform window grew from 6e-7 at T = 3 to 1.9e-5 at T = 136 and 7.65e-5 at T = 512 - a difference of definition, not an error -, and the
waveform's gate grew with it, to 1.5e-4 at T = 512.  With the positions kept, the oracle's worst window is at most 4.4e-7 on the waveform and
5.1e-7 on every other FilterNet block at every length here (profiles/wave_edges.txt), so the 3e-6 floor decides for ALL ten tensors; no gate
is wider than it was.  tests/test_wave_truth_host.py proves the restated positions against F.interpolate, these figures and the gate's
sensitivity with the oracle alone.

What the gate sees: an error of 1e-4 of the row's rms in two columns reads 2.5e-5 in its window.  That trips the gate on every compared tensor at
every shape here, the waveform included - the only view of ups[4] (filter_up24s.hip: two up24s_kernel launches on 250-output tiles, the second
with a 9 + 27 + 3-column halo, c5 and the k7 output conv folded in), which is no parity tap.  The gate also refuses an interpolation that is
MORE exact than ATen's - a per-phase lambda table (dst % 5) in place of lerp_coord differs from the reference by 1.1e-5 per window at T = 43 -
from T = 26 on.

Each case prints one `[edge]` line: the window closest to (or furthest beyond) its gate with its block, row and first column, that block's
whole-tensor figure, and per tensor group the worst GPU and the worst oracle window.  Each of (a), (b), (c) also bumps the last two columns of
one GPU block - in (a) and (b) also of the waveform - by 1e-4 of its rms ON THE HOST and requires the gate to trip."""
import pytest
import torch

from helpers import FILTER_EDGE_LENGTHS, WIDE_FILM_SHAPES, _bump_trips, _gate_case, oracle_one_thread, rel_rms, state_dicts
from helpers import filter_edge_inputs as _filter_inputs, filter_edge_oracle as _filter_oracle, filter_named as _named, sd64 as _sd64
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


# ------------------------------------------------------------------------------------------------ FilterNet
def _filter_gpu(eng, inputs):
    return _named(*eng.filter_net(*[x.to(DEV) for x in inputs], blocks=True))


@pytest.mark.parametrize("T", FILTER_EDGE_LENGTHS)
def test_filter_net_blocks_per_window_at_tile_edges(gen, T):
    """(a) B = 1, all five `skips`, ups[0..3] and the waveform.  Levels run at 2T, 6T, 24T (384 / 192 / 96 channels), 96T (48) and 480T (24)
    columns.  Tile constants: U24S_WA = 250, down0 W = 254, D24F::W = 244, kBN48 = 128 (128 - 2 db outputs for the pair kernel), CS2::BN =
    FS2::BN = 256 with FS2T<7> = 224, conv3s 128.

      T   what it puts on a seam
      1   ups.4 (480T columns, 250-output tiles in both up24s halves): 480 columns, one full tile and one of 230.  Every coarser level is
          shorter than its halo
      3   every level of 96 channels and up (6, 18 and 72 columns) is shorter than two 27-column halos: most taps of the 9- and 27-dilated
          convs land on replicate padding
      9   down0s tail of 2 columns (4320 = 17 x 254 + 2)
     12   ups.4: 5760 = 23 x 250 + 10, the smallest possible tail (480T mod 250 = 10 at T = 12 mod 25), shorter than the second half's
          39-column halo
     25   ups.4: 12 000 = 48 x 250, a whole number of tiles: the last tile's right halo is all replicate padding
     26   conv48p's 124-output tiles (Downsample 2's c1 -> c2 pair, 128 - 2 x 2, at 24T columns) tail of 4 (624 = 5 x 124 + 4)
     28   down24f tail of 4 columns (96T = 2688 = 11 x 244 + 4): so far under the whole-tensor gate only
     37   ups.4: 17 760 = 71 x 250 + 10 again, with 6T = 222 still below the conv_s2 / film_s2 switch at 258
     43   6T = 258: the first length at which the 192-channel level takes conv_s2 / film_s2 (224 variant), with a 2-column conv_s2 tail.
          2T = 86 and 24T = 1032 on the other paths
     65   conv3s 128-column tails of 2 (2T = 130, the FiLM narrow tile) and of 6 (6T = 390, Downsample's c3 on conv3s)
    127   one column pair below every boundary: 2T = 254 stays on conv3s.  6T = 762 and 24T = 3048 leave film_s2's 256-column tiles 250 and
          232 wide.  480T = 240 full down0s tiles
    128   every level of 96 channels and up is a whole number of 256-column tiles, and the 256-wide film_s2 variant runs on all three: the
          only block-wise check of it at 384 channels
    129   tails of 2, 6 and 24 columns for conv_s2, and the 224-wide film_s2 variant on all three levels
    136   down0s tail of 2 behind 257 full tiles, and the conv48p (122 outputs) tail of 2
    512   ups.4: 245 760 = 983 x 250 + 10, far out where one ulp of `src` is 2^-8 of a sample (the plain fp64 truth allowed 1.5e-4 here).  The
          three coarser levels are whole 256-column tiles

    Before T = 1, 12, 25, 37 and 512 the ups.4 tails were 30 .. 230 columns, never shorter than the halo and never 0."""
    inputs = _filter_inputs(1, T)
    truth, ref = _filter_oracle(inputs)
    gpu = _filter_gpu(gen.decoder.engine(DEV), inputs)
    fails, gates = _gate_case(f"filter_net B=1 T={T}", gpu, truth, ref)
    assert not fails, f"T={T}: " + "; ".join(fails)
    assert _bump_trips(gpu, truth, gates, "ups[2]"), "1e-4 x rms on the last two columns of ups[2] must trip the window gate"
    assert _bump_trips(gpu, truth, gates, "wave"), "1e-4 x rms on the last two columns of the waveform must trip the window gate"


@pytest.mark.parametrize("B,T", WIDE_FILM_SHAPES)
def test_wide_film_tile_per_window_and_batch_invariance(gen, B, T):
    """(b) conv3s's 96 x 256 FiLM tile (scale and shift as two phases on one extra accumulator pair) runs only for an equal-length batch of
    short utterances: mb * ceil(len / 256) * B >= 256 tiles at len < 256.  B = 64, T = 100: the 384-channel level (200 columns, 4 x 64
    tiles).  B = 256, T = 5: all three levels (10, 30, 120 columns).  It is the one FiLM kernel choice that looks at B; an utterance
    converts to the same samples in every batch, so rows 0, 1, B / 2, B - 1 must pass the window gate AND equal their
    own B = 1 calls bit for bit."""
    rows = [0, 1, B // 2, B - 1]
    inputs = _filter_inputs(B, T)
    sub = [x[rows] for x in inputs]
    truth, ref = _filter_oracle(sub)
    eng = gen.decoder.engine(DEV)
    idx = torch.tensor(rows, device=DEV)
    gpu = {k: v.index_select(0, idx) for k, v in _filter_gpu(eng, inputs).items()}
    differ = []
    for i, r in enumerate(rows):
        one = _filter_gpu(eng, [x[r:r + 1] for x in inputs])
        differ += [f"{k} row {r}" for k, v in one.items() if not torch.equal(v[0], gpu[k][i])]
    fails, gates = _gate_case(f"filter_net wide FiLM tile B={B} T={T} rows {rows}" + (" [differs from B = 1: " + ", ".join(differ) + "]" if differ else " [rows equal their B = 1 calls]"),
                              gpu, truth, ref)
    assert not fails, f"B={B} T={T}: " + "; ".join(fails)
    assert _bump_trips(gpu, truth, gates, "ups[0]"), "1e-4 x rms on the last two columns of ups[0] must trip the window gate"
    assert _bump_trips(gpu, truth, gates, "wave"), "1e-4 x rms on the last two columns of the waveform must trip the window gate"
    assert not differ, f"B={B} T={T}: the batched call differs from the rows' own B = 1 calls in " + ", ".join(differ)


# ------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("B,T", [(3, 32), (3, 33), (3, 64), (3, 65), (1, 1024), (1, 1025)])
def test_encoder_per_window_at_tile_edges(gen, B, T):
    """(c) ssl and pitch logits.  (3, 32) / (3, 33): cnx1<C, 1> against <C, 2>, a 1-column tile tail, and flat gemm_s2 tiles that straddle
    utterances.  (3, 64) / (3, 65): a 1-column tail for cnx1 / cnx2 at 64 columns.  (1, 1024) / (1, 1025): 16 against 17 GRN tile sums,
    added inline (CNX_GP_INLINE = 16) against grn_tiles_kernel.  The oracle's fp32 windows are 5.5e-7 .. 5.8e-7 on ssl and 3.5e-8 .. 3.6e-8
    on the logits (profiles/tile_edges.txt), so the 3e-6 floor decides.  f0 within the 2e-6 of the headline test."""
    e64, _d64 = _sd64()
    enc_sd, _dec_sd = state_dicts(0)
    spec = R.spectrogram(synth.synth_wave(B, 480 * T, seed=2000 + T))
    s64 = spec.double()
    truth = {"ssl": R.ssl_features(e64, s64), "logits": R.pitch_logits(e64, s64)}
    f0_truth = R.pitch_decode(truth["logits"])
    with oracle_one_thread():
        ref = {"ssl": R.ssl_features(enc_sd, spec), "logits": R.pitch_logits(enc_sd, spec)}
    ssl, f0, logits = gen.encoder.engine(DEV).encoder(spec.to(DEV), want_logits=True)
    gpu = {"ssl": ssl, "logits": logits}
    e_f0 = rel_rms(f0.cpu(), f0_truth)
    fails, gates = _gate_case(f"encoder B={B} T={T}", gpu, truth, ref, extra=f"; f0 rel rms vs the fp64 truth {e_f0:.2e}")
    assert not fails, f"B={B} T={T}: " + "; ".join(fails)
    assert _bump_trips(gpu, truth, gates, "ssl"), "1e-4 x rms on the last two columns of ssl must trip the window gate"
    assert e_f0 <= 2e-6


# ------------------------------------------------------------------------------------------------ ragged
def test_ragged_rows_at_checked_lengths_equal_their_own_calls(gen):
    """(d) One ragged convert with 43, 65, 129 and 136 frames (rows 1 and 3 end 7 samples early): the RAG kernels - which always run
    film_s2's 256-wide variant - have 2-column tails here.  Every row equals its own B = 1 conversion bit for bit, whose blocks (a) has
    compared with the truth at these very lengths; the padding behind an utterance is zero."""
    frames = [43, 65, 129, 136]
    lens = [480 * f - (7 if b in (1, 3) else 0) for b, f in enumerate(frames)]
    wf = torch.zeros(len(frames), 480 * max(frames))
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=400 + b)[0]
    wf = wf.to(DEV)
    tgt = synth.synth_index(500, seed=2).to(DEV)
    angle = synth.synth_angle(len(frames), max(frames), 13).to(DEV)
    out = gen.convert(wf, tgt, 1.0, noise_angle=angle, lengths=lens)
    assert out.shape == (len(frames), 480 * max(frames)) and torch.isfinite(out).all()
    for b, f in enumerate(frames):
        one = gen.convert(wf[b:b + 1, :lens[b]], tgt, 1.0, noise_angle=angle[b:b + 1, :, :f].contiguous())
        assert one.shape == (1, 480 * f)
        assert torch.equal(out[b, :480 * f], one[0]), f"{f} frames"
        assert not out[b, 480 * f:].any(), f"{f} frames: the padding behind the utterance must be zero"
    print(f"[edge] ragged convert, frames {frames} (rows 1 and 3 end 7 samples early): every row equals its own B = 1 conversion, zeros behind")
