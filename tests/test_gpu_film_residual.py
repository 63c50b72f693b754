"""film_s2's tile end, bit for bit against the build before its residual reads were batched and moved ahead of the tile end.

The change moves only WHEN a tile's residual rows are requested (film_s2.h): a column's arithmetic and its order stay what they were, so
FilterNet's outputs may not move by one bit.  The fixtures under tests/golden/ (film_residual_*.npy: the waveforms as full float32 arrays;
film_residual_sums.json: per block output the 64-bit sum of its elements' bit patterns) were recorded from the parent build with this file's
own `--record` mode; the tests run the same calls and require `torch.equal`.

Shapes: the smallest at which each film_s2 instantiation runs and can still go wrong (levels run at 2T / 6T / 24T columns on 384 / 192 /
96 channels; the first half of an Upsample reads its residual interpolated from the low-rate tensor, the second half directly).

    B  T    what runs
    2  43   6T = 258 and 24T = 1032: the 192- and 96-channel levels on the 224-wide variant, tails of 34 and 136 columns (2T = 86 stays
            on the narrow conv3s tile)
    2  129  the 224-wide variant on all three levels, tails of 34 / 102 / 184 columns behind conv_s2's 2 / 6 / 24
    1  128  whole 256-column tiles: the 256-wide variant on all three levels
    ragged  one convert with 43 and 129 frames (row 1 ends 7 samples early): the RAG instantiations, 2-column tails, the utterance's
            first column riding in the lane offsets

Every call ends an utterance inside a tile, so the clamped columns tc = len - 1 and the interpolated residual's last low-rate frame
(i1 = i0 = n - 1) are covered."""
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import GOLDEN, state_dicts
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(2, 43), (2, 129), (1, 128)]
RAGGED_FRAMES = [43, 129]
SUMS = os.path.join(GOLDEN, "film_residual_sums.json")


def _generator():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def sums():
    with open(SUMS) as f:
        return json.load(f)


def _filter_inputs(B, T):
    g = torch.Generator().manual_seed(7000 + 10 * T + B)
    L = 480 * T
    content = torch.randn(B, 768, T, generator=g) * 0.5
    f0 = 80.0 + 200.0 * torch.rand(B, 1, T, generator=g)
    source = torch.randn(B, 16, L, generator=g) * 0.3
    energy = torch.rand(B, 1, L, generator=g)
    return content, f0, energy, source


def _filter_gpu(eng, inputs):
    wave, skips, ups = eng.filter_net(*[x.to(DEV) for x in inputs], blocks=True)
    d = {f"downs[{i}]": s for i, s in enumerate(skips)}
    d.update({f"ups[{i}]": u for i, u in enumerate(ups[:4])})
    return wave, d


def _bit_sum(t):
    """64-bit sum of the elements' bit patterns (each taken as an unsigned 32-bit number)."""
    return int((t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sum())


def _ragged(gen):
    lens = [480 * f - (7 if b == 1 else 0) for b, f in enumerate(RAGGED_FRAMES)]
    wf = torch.zeros(len(lens), 480 * max(RAGGED_FRAMES))
    for b, n in enumerate(lens):
        wf[b, :n] = synth.synth_wave(1, n, seed=700 + b)[0]
    tgt = synth.synth_index(500, seed=2).to(DEV)
    angle = synth.synth_angle(len(lens), max(RAGGED_FRAMES), 17).to(DEV)
    return gen.convert(wf.to(DEV), tgt, 1.0, noise_angle=angle, lengths=lens)


def _wave_file(tag):
    return os.path.join(GOLDEN, f"film_residual_{tag}.npy")


@pytest.mark.parametrize("B,T", CASES)
def test_filter_net_equals_the_recorded_bits(gen, sums, B, T):
    wave, blocks = _filter_gpu(gen.decoder.engine(DEV), _filter_inputs(B, T))
    want = torch.from_numpy(np.load(_wave_file(f"B{B}_T{T}")))
    assert wave.shape == want.shape
    got = {k: _bit_sum(v) for k, v in blocks.items()}
    differ = [k for k, v in sums[f"B{B}_T{T}"].items() if got[k] != v]
    print(f"[film residual] B={B} T={T}: waveform {'equal' if torch.equal(wave.cpu(), want) else 'DIFFERS'}, "
          f"{len(got) - len(differ)} of {len(got)} block sums equal" + (", differing: " + ", ".join(differ) if differ else ""))
    assert not differ, f"B={B} T={T}: block outputs moved: " + ", ".join(differ)
    assert torch.equal(wave.cpu(), want), f"B={B} T={T}: the waveform moved"


def test_ragged_convert_equals_the_recorded_bits(gen):
    out = _ragged(gen)
    want = torch.from_numpy(np.load(_wave_file("ragged")))
    assert out.shape == want.shape
    assert torch.equal(out.cpu(), want), "the ragged conversion moved"


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    g_ = _generator()
    rec = {}
    for B_, T_ in CASES:
        wave_, blocks_ = _filter_gpu(g_.decoder.engine(DEV), _filter_inputs(B_, T_))
        np.save(_wave_file(f"B{B_}_T{T_}"), wave_.cpu().numpy())
        rec[f"B{B_}_T{T_}"] = {k: _bit_sum(v) for k, v in blocks_.items()}
    np.save(_wave_file("ragged"), _ragged(g_).cpu().numpy())
    with open(SUMS, "w") as f_:
        json.dump(rec, f_, indent=1, sort_keys=True)
        f_.write("\n")
    print("recorded", sorted(rec), "and the ragged conversion under", GOLDEN)
