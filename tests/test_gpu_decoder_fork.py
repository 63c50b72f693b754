"""The decoder's fork (csrc/decoder.hip run_decoder): FilterNet's content-only front - the input contraction and Upsample 0's c1 - runs
on the context's side stream, off FilterNet's serial chain, and is joined in front of Upsample 0's FiLM launch.

An eager call forks; the same call under stream capture keeps one chain (the library never forks while captured).  Where the launches
sit must not change a bit, so every check here is torch.equal: forked against unforked, a ragged batch against its rows one by one, and
calls that reuse one workspace back to back - a side chain that is joined too late, or not at all, shows as a difference there.

No test here makes a call that fails behind the fork: the only refusal in run_filter (level lengths that do not divide by the next
Downsample factor) cannot be reached through the public entries - every length is 480 T - and the kernels' own preconditions hold
for the fixed architecture."""
import pytest
import torch

from helpers import state_dicts
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _generator():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _generator()


@pytest.fixture(scope="module")
def tgt():
    return synth.synth_index(256, seed=2).to(DEV)


def _replayed(call):
    """`call` once eagerly (weights packed, workspace grown), then captured and replayed -> the replay's outputs"""
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    return out


# T = 140: level 0 is 280 columns - one full and one partial 256-column tile, the pipelined c1 with the pre-split hand-over;
# T = 28: 56 columns, below one tile - c1's plain form, whose launch raises h's |max| slot
@pytest.mark.parametrize("T", [140, 28])
def test_forked_convert_equals_the_captured_single_chain(gen, tgt, T):
    wf = synth.synth_wave(2, T * 480, seed=60 + T).to(DEV)
    angle = synth.synth_angle(2, T, 61).to(DEV)      # the phases are passed in: a seeded draw is refused under capture
    eager = gen.convert(wf, tgt, 1.0, noise_angle=angle)
    cap = _replayed(lambda: gen.convert(wf, tgt, 1.0, noise_angle=angle))
    assert eager.shape == (2, T * 480) and torch.isfinite(eager).all() and eager.abs().max() > 0
    assert torch.equal(eager, cap), f"T = {T}: the forked call differs from the single chain by up to {float((eager - cap).abs().max()):.3e}"


def test_ragged_batch_equals_its_rows_one_by_one(gen, tgt):
    frames = [28, 140, 200]      # one length class below a 256-column tile at level 0, two above it (another batch of the same call)
    lens = [480 * f for f in frames]
    wf = torch.zeros(3, max(lens))
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=70 + b)[0]
    wf = wf.to(DEV)
    angle = synth.synth_angle(3, max(frames), 71).to(DEV)
    out = gen.convert(wf, tgt, -0.5, noise_angle=angle, lengths=lens)
    for b, f in enumerate(frames):
        one = gen.convert(wf[b:b + 1, :lens[b]].contiguous(), tgt, -0.5, noise_angle=angle[b:b + 1, :, :f].contiguous())
        assert torch.equal(out[b, :lens[b]], one[0]), f"utterance {b} ({f} frames): ragged batch != its own B = 1 call"
        assert not out[b, lens[b]:].any()


def test_decoder_stage_call_forked_equals_captured(gen):
    """The stage entry measures its own |max| slots (no bounds from the caller): x0's slot is then set in front of the fork, where c1 on
    the side stream finds it.  The entry has no taps of FilterNet's blocks; h0 reaches the waveform through every later launch, and
    `source` covers the first join (the harmonic rows)."""
    B, T = 2, 140
    g = torch.Generator().manual_seed(80)
    content = torch.randn(B, 768, T, generator=g).to(DEV)
    f0 = (torch.rand(B, 1, T, generator=g) * 200 + 80).to(DEV)
    f0[:, :, 50:60] = 0.0      # an unvoiced stretch
    energy = torch.rand(B, 1, T * 480, generator=g).to(DEV)
    angle = synth.synth_angle(B, T, 81).to(DEV)
    eng = gen.engine(DEV)
    eager = eng.decoder(content, f0, energy, angle, stages=True)
    cap = _replayed(lambda: eng.decoder(content, f0, energy, angle, stages=True))
    for name, a, b in zip(("wave", "amps", "kernel", "source"), eager, cap):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{name}: the forked stage call differs from the single chain"
    assert torch.equal(eager[0], eng.decoder(content, f0, energy, angle)), "the waveform-only entry"


def test_back_to_back_calls_share_one_workspace(gen, tgt):
    """Nothing waits between the calls: the next call's first writes land in the workspace the previous call's side chain wrote into."""
    T = 140
    wfs = [synth.synth_wave(2, T * 480, seed=90 + i).to(DEV) for i in range(3)]
    angle = synth.synth_angle(2, T, 91).to(DEV)
    gen.convert(wfs[0], tgt, 0.0, noise_angle=angle)      # the workspace is grown
    torch.cuda.synchronize()
    outs = [gen.convert(w, tgt, 0.0, noise_angle=angle) for w in wfs]
    last = gen.convert(wfs[0], tgt, 0.0, noise_angle=angle)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], last), "the first call again, behind two others"
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    fresh = _generator()
    for w, o in zip(wfs, outs):
        assert torch.equal(fresh.convert(w, tgt, 0.0, noise_angle=angle), o), "a fresh engine, one call at a time"
