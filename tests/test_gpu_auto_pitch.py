"""Automatic pitch on the device: the row-wise pitch register (a radix select: the lower median of the voiced frames, bit for bit
torch.median), the shift onto a target register, and convert with that shift found inside the call (tvc_pitch_match_f32,
tvc_convert_auto_f32, tvc_convert_ragged_auto_f32; Generator.convert(auto_pitch=...)).

Contracts: the median's bits and the voiced count equal torch.median(row[row > 0]) on the CPU; rows of one launch do not see each other;
the shift is the fp64 formula rounded once; an automatic convert equals, bit for bit, the existing per-row-shift call fed the shifts it
reports; a captured call follows a new utterance without a new capture."""
import numpy as np
import pytest
import torch

from helpers import state_dicts
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 70001]      # around a wave, a workgroup pass, the 4-deep unrolled walk; one long row
PATTERNS = ["unvoiced", "one_voiced", "even_count", "all_equal", "last_bits", "exponents", "nan_negative"]


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


def _engine():
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _spread(n, g):
    return torch.exp(torch.empty(n).uniform_(float(np.log(20.1)), float(np.log(3000.0)), generator=g))      # 20.1 .. 3000 Hz: eight exponents


def _row(pattern, n, seed):
    g = torch.Generator().manual_seed(seed)
    if pattern == "unvoiced":
        return torch.zeros(n)
    if pattern == "one_voiced":
        x = torch.zeros(n)
        x[n // 2] = 123.4
        return x
    if pattern == "even_count":      # the lower of the two middle values; a row of one frame has no even count but zero
        x = torch.zeros(n)
        k = n - n % 2
        x[torch.randperm(n, generator=g)[:k]] = torch.empty(k).uniform_(50.0, 400.0, generator=g)
        return x
    if pattern == "all_equal":
        return torch.full((n,), 220.0)
    if pattern == "last_bits":       # only the last radix pass can tell them apart
        base = torch.tensor([220.0]).view(torch.int32)
        return (base + torch.randint(0, 4, (n,), generator=g, dtype=torch.int32)).view(torch.float32)
    x = _spread(n, g)
    if pattern == "nan_negative":
        u = torch.rand(n, generator=g)
        x[u < 0.15] = float("nan")
        x[(u >= 0.15) & (u < 0.3)] *= -1.0
        x[(u >= 0.3) & (u < 0.4)] = 0.0
    return x


def _reference(row):
    """(bits of torch.median over the voiced values - of 0.0 without one -, their count), on the CPU"""
    v = row[row > 0]
    med = torch.median(v) if v.numel() else torch.zeros(())
    return int(med.view(torch.int32)), v.numel()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_selection_is_torch_median(pattern):
    eng = _engine()
    for i, n in enumerate(LENGTHS):
        row = _row(pattern, n, 100 + i)
        med, voiced, shift, _ = eng.pitch_match(row[None].to(DEV), pitch_shift=1.5)
        want_bits, want_n = _reference(row)
        assert int(voiced[0]) == want_n, f"{pattern}, {n} frames: {int(voiced[0])} voiced, torch counts {want_n}"
        assert int(med.cpu().view(torch.int32)[0]) == want_bits, f"{pattern}, {n} frames: median {float(med[0])!r}, torch.median {_reference(row)}"
        assert float(shift[0]) == 1.5      # no target: the offset


def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


def test_rows_of_one_launch_and_the_shift():
    """Rows of 3, 64, 17 (no voiced frame), 1, 257 and 28 frames in one launch, poison in front of the first and behind the last: every row
    equals the launch of that row alone.  Then the shift: within one fp32 ulp of the fp64 formula (two fp64 evaluations rounded once cannot
    differ by more), the offset exactly for a row without a voiced frame or a target <= 0 / NaN, and the shifted f0 is
    tvc_shift_frequency_f32 of the row by the reported shift."""
    eng = _engine()
    lens = [3, 64, 17, 1, 257, 28]
    g = torch.Generator().manual_seed(7)
    rows = [_spread(n, g) * (1.0 + 0.1 * i) for i, n in enumerate(lens)]
    rows[2] = -rows[2]                                       # an unvoiced row between voiced ones
    rows[4][torch.rand(257, generator=g) < 0.3] = 0.0
    head, tail = 5, 7
    packed = torch.cat([torch.full((head,), 1e30)] + rows + [torch.full((tail,), 1e30)]).to(DEV)
    start = [head]
    for n in lens:
        start.append(start[-1] + n)
    target = torch.tensor([300.0, 0.0, 150.0, float("nan"), 97.3, 440.0], device=DEV)
    offs = [0.0, 1.0, -2.0, 3.0, 0.25, -0.5]
    med, voiced, shift, f0s = eng.pitch_match(packed, start, target, offs, want_shifted=True)
    assert not f0s[:head].any() and not f0s[-tail:].any(), "columns outside every row were written"
    for b, n in enumerate(lens):
        m1, v1, s1, f1 = eng.pitch_match(rows[b][None].to(DEV), None, target[b:b + 1].contiguous(), offs[b], want_shifted=True)
        want_bits, want_n = _reference(rows[b])
        assert int(v1[0]) == want_n and int(m1.cpu().view(torch.int32)[0]) == want_bits
        assert int(voiced[b]) == int(v1[0]) and torch.equal(med[b:b + 1], m1), f"row {b}: its neighbours leaked into it"
        assert torch.equal(shift[b:b + 1], s1) and torch.equal(f0s[start[b]:start[b + 1]], f1[0], ), f"row {b}"
        tg = float(target[b])
        if want_n == 0 or not tg > 0:
            assert float(shift[b]) == offs[b], f"row {b}: {float(shift[b])!r} is not the offset"
        else:
            want = np.float32(np.float64(offs[b]) + 12.0 * np.log2(np.float64(np.float32(tg)) / np.float64(med[b].item())))
            d = int(_ulps(shift[b:b + 1].cpu(), torch.tensor([want]))[0])
            print(f"[auto pitch] row {b}: shift {float(shift[b])!r}, numpy fp64 {float(want)!r}: {d} ulp")
            assert d <= 1, f"row {b}: {d} ulps from the fp64 formula"
        assert torch.equal(f0s[start[b]:start[b + 1]], eng.shift_frequency(packed[start[b]:start[b + 1]], float(shift[b])))
    assert int(voiced[2]) == 0 and float(med[2]) == 0.0


def _registers(gen, wf, lens=None):
    """pitch_register of Generator.encode's f0, row by row over each row's own frames"""
    from tinyvc_amd.module.tinyvc.feature_retrieval import pitch_register
    out = []
    for b in range(wf.shape[0]):
        _z, f0 = gen.encode(wf[b:b + 1, :(lens[b] if lens else wf.shape[1])].to(DEV))
        out.append(pitch_register(f0))
    return out


def _check_shifts(gen, wf, lens, target_hz, offs, sh):
    """voiced rows, pairwise different shifts (no vacuous pass), and agreement with the register of `encode`'s f0.  `encode` and `convert`
    decode f0 from the same weights under different fp16-split scales (a measured against a bounded |max|); the project holds either
    within 7e-6 of the fp64 truth (test_gpu_parity.py), an order statistic moves by no more than its inputs, and 12 log2(1 + 1.4e-5) =
    2.4e-4 semitones: 3e-4 with the fp32 rounding of a shift below 32."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import semitones_between
    regs = _registers(gen, wf, lens)
    got = sh.cpu().tolist()
    for b, reg in enumerate(regs):
        assert int(reg.voiced[0]) > 0, f"row {b} has no voiced frame"
        want = offs[b] + semitones_between(float(reg.median_hz[0]), target_hz[b])
        print(f"[auto pitch] row {b}: register {float(reg.median_hz[0]):.3f} Hz over {int(reg.voiced[0])} frames, shift {got[b]:+.6f}, from encode {want:+.6f}")
        assert abs(got[b] - want) <= 3e-4, f"row {b}: shift {got[b]} against {want} from encode's f0"
    assert len(set(got)) == len(got), f"the row shifts do not differ pairwise: {got}"


def test_convert_equal_batch(gen):
    """B = 3 at 50 frames against one shared index: the automatic call == convert with the reported shifts as host shifts."""
    B, T = 3, 50
    wf = synth.synth_wave(B, T * 480, seed=11).to(DEV)
    tgt = synth.synth_index(300, seed=12).to(DEV)
    angle = synth.synth_angle(B, T, 13).to(DEV)
    target_hz, offs = [220.0, 110.0, 330.0], [0.5, -1.0, 2.0]
    out, sh = gen.convert(wf, tgt, offs, noise_angle=angle, auto_pitch=torch.tensor(target_hz, device=DEV), return_shift=True)
    _check_shifts(gen, wf, None, target_hz, offs, sh)
    ref = gen.convert(wf, tgt, sh.cpu().tolist(), noise_angle=angle)
    assert torch.equal(out, ref), "auto-pitch convert != the per-row-shift call fed its shifts"
    # a float register, a scalar offset, no shifts asked for: the same path
    one = gen.convert(wf, tgt, 0.5, noise_angle=angle, auto_pitch=220.0)
    assert torch.equal(one[0], out[0])


def test_convert_own_register_is_the_offset(gen):
    """A register equal to the row's own median (pitch_register of `encode`'s f0), offset 2.0: log2(1) = 0, the shift is the offset exactly
    and the waveform is the plain per-row call's with shift 2.0, bit for bit."""
    B, T = 2, 50
    wf = synth.synth_wave(B, T * 480, seed=17).to(DEV)
    tgt = synth.synth_index(300, seed=12).to(DEV)
    angle = synth.synth_angle(B, T, 19).to(DEV)
    regs = torch.cat([r.median_hz for r in _registers(gen, wf)])
    out, sh = gen.convert(wf, tgt, 2.0, noise_angle=angle, auto_pitch=regs, return_shift=True)
    print(f"[auto pitch] own-register shifts {sh.tolist()}")
    assert bool((sh == 2.0).all()), f"encode's register is not the in-call median: shifts {sh.tolist()}"
    assert torch.equal(out, gen.convert(wf, tgt, [2.0] * B, noise_angle=angle))


def test_convert_ragged_two_indices_and_blend(gen):
    """A ragged batch of 8, 30, 60 and 140 frames (the four length classes) against two distinct indices carrying their registers
    (auto_pitch=True); an equal batch against two distinct indices; a Blend of two terms with an explicit register."""
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, PitchRegister
    a, b = synth.synth_index(300, seed=21).to(DEV), synth.synth_index(6000, seed=22).to(DEV)
    a.pitch_register = PitchRegister(torch.tensor([240.0], device=DEV), torch.tensor([900], dtype=torch.int32, device=DEV))
    b.pitch_register = PitchRegister(torch.tensor([95.0], device=DEV), torch.tensor([700], dtype=torch.int32, device=DEV))
    frames = [8, 30, 60, 140]
    lens = [480 * f - (13 if i % 2 else 0) for i, f in enumerate(frames)]
    B, Lmax = len(frames), 480 * max(frames)
    wf = torch.zeros(B, Lmax)
    for r, n in enumerate(lens):
        wf[r, :n] = synth.synth_wave(1, n, seed=700 + 3 * r)[0] if r % 2 == 0 else synth.synth_wave(2, n, seed=700 + 3 * r)[1]
    wf = wf.to(DEV)
    angle = synth.synth_angle(B, max(frames), 23).to(DEV)
    tg = [a, b, b, a]
    offs = [0.0, 1.0, -1.5, 0.25]
    out, sh = gen.convert(wf, tg, offs, noise_angle=angle, lengths=lens, auto_pitch=True, return_shift=True)
    _check_shifts(gen, wf, [480 * f for f in frames], [240.0, 95.0, 95.0, 240.0], offs, sh)
    ref = gen.convert(wf, tg, sh.cpu().tolist(), noise_angle=angle, lengths=lens)
    assert torch.equal(out, ref), "ragged auto-pitch convert != the per-row-shift call fed its shifts"
    # two distinct indices, equal lengths
    wf2 = synth.synth_wave(2, 50 * 480, seed=31).to(DEV)
    angle2 = synth.synth_angle(2, 50, 32).to(DEV)
    out2, sh2 = gen.convert(wf2, [a, b], 0.0, noise_angle=angle2, auto_pitch=True, return_shift=True)
    _check_shifts(gen, wf2, None, [240.0, 95.0], [0.0, 0.0], sh2)
    assert torch.equal(out2, gen.convert(wf2, [a, b], sh2.cpu().tolist(), noise_angle=angle2))
    # a blend of the two, its register given: equal and ragged
    blend = Blend([a, b], [0.6, 0.4])
    out3, sh3 = gen.convert(wf2, blend, [0.0, -1.0], noise_angle=angle2, auto_pitch=torch.tensor([180.0, 200.0], device=DEV), return_shift=True)
    _check_shifts(gen, wf2, None, [180.0, 200.0], [0.0, -1.0], sh3)
    assert torch.equal(out3, gen.convert(wf2, blend, sh3.cpu().tolist(), noise_angle=angle2))
    out4, sh4 = gen.convert(wf, Blend([a, b], [0.6, 0.4]), 0.5, noise_angle=angle, lengths=lens, auto_pitch=170.0, return_shift=True)
    assert torch.equal(out4, gen.convert(wf, Blend([a, b], [0.6, 0.4]), sh4.cpu().tolist(), noise_angle=angle, lengths=lens))


def test_captured_call_follows_the_input(gen):
    """One B = 1 automatic convert captured as a graph, replayed on a second utterance written into the same input buffer: shifts and
    waveform are the eager call's on that utterance - the starts and offsets are arguments, the f0 and the register are read on the device."""
    T = 50
    tgt = synth.synth_index(300, seed=41).to(DEV)
    first, second = synth.synth_wave(1, T * 480, seed=42).to(DEV), synth.synth_wave(2, T * 480, seed=43)[1:2].to(DEV)
    angle = synth.synth_angle(1, T, 44).to(DEV)
    reg = torch.tensor([205.0], device=DEV)
    buf = first.clone()
    gen.convert(buf, tgt, 1.0, noise_angle=angle, auto_pitch=reg, return_shift=True)      # eager once: weights packed, index prepared, workspace grown
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        wave, sh = gen.convert(buf, tgt, 1.0, noise_angle=angle, auto_pitch=reg, return_shift=True)
    buf.copy_(second)
    g.replay()
    torch.cuda.synchronize()
    want, want_sh = gen.convert(second, tgt, 1.0, noise_angle=angle, auto_pitch=reg, return_shift=True)
    other, other_sh = gen.convert(first, tgt, 1.0, noise_angle=angle, auto_pitch=reg, return_shift=True)
    assert not torch.equal(want_sh, other_sh), "the two utterances share a register: the case shows nothing"
    assert torch.equal(sh, want_sh) and torch.equal(wave, want), "the replay did not follow the new utterance"
    assert not torch.equal(wave, other)


CLIP_LENS = [24000, 31011, 19500]


def test_build_index_carries_the_register(gen):
    from tinyvc_amd.module.tinyvc.feature_retrieval import build_index
    wf = torch.zeros(len(CLIP_LENS), max(CLIP_LENS))
    for i, n in enumerate(CLIP_LENS):
        wf[i, :n] = synth.synth_wave(1, n, seed=50 + i)[0]
    index = build_index(gen, wf.to(DEV), list(CLIP_LENS), stride=4, size=30, perm=torch.randperm(41, generator=torch.Generator().manual_seed(1)))      # 13 + 17 + 11 strided frames
    _ssl, f0, _pre = gen.encode_packed(wf.to(DEV), list(CLIP_LENS))
    f0 = f0.cpu()
    v = f0[f0 > 0]
    reg = index.pitch_register
    assert v.numel() > 0 and int(reg.voiced[0]) == v.numel()
    assert torch.equal(reg.median_hz.cpu(), torch.median(v)[None])


def test_extract_index_writes_the_sidecar_and_the_same_index(tmp_path):
    """`index.pt` is, byte for byte, what the recipe without the register writes for the same --seed (the clip-by-clip loop and `assemble`,
    run here as they stood); the sidecar holds the register of every frame of the clips it used."""
    import extract_index
    from tinyvc_amd.module import utils
    from tinyvc_amd.module.tinyvc import Encoder
    d = tmp_path / "clips"
    d.mkdir()
    torch.save(synth.synth_state_dict("encoder"), tmp_path / "encoder.pt")
    for i, n in enumerate(CLIP_LENS):
        audio_io.save(str(d / f"{i}.wav"), synth.synth_wave(1, n, seed=50 + i), 24000)
    common = ["--dataset-cache", str(d), "-encp", str(tmp_path / "encoder.pt"), "-size", "30", "-d", DEV, "--seed", "7"]
    assert extract_index.main(common + ["-o", str(tmp_path / "index.pt")]) == 0
    enc = Encoder()
    enc.load_state_dict(torch.load(tmp_path / "encoder.pt", map_location="cpu"))
    enc = enc.eval().to(DEV)
    files = sorted(str(p) for p in d.glob("*.wav"))
    g = torch.Generator().manual_seed(7)
    feats, f0s, total = [], [], 0
    for i in torch.randperm(len(files), generator=g).tolist():
        wf, sr = audio_io.load(files[i])
        spec = utils.spectrogram(utils.autopad_waveform(wf.to(DEV).mean(dim=0, keepdim=True)), enc.n_fft, enc.hop_size)
        z, f0 = enc.infer(spec)
        feats.append(z.cpu()[:, :, ::4])
        f0s.append(f0.reshape(-1).cpu())
        total += feats[-1].shape[2]
        if total > 30:
            break
    (tmp_path / "parent").mkdir()      # (torch.save writes the file's base name into the archive: the same name in another folder)
    torch.save(extract_index.assemble(feats, 30, g, False), tmp_path / "parent" / "index.pt")
    assert open(tmp_path / "index.pt", "rb").read() == open(tmp_path / "parent" / "index.pt", "rb").read()
    side = torch.load(str(tmp_path / "index.pt") + ".f0.pt")
    f0 = torch.cat(f0s)
    v = f0[f0 > 0]
    assert side == {"median_hz": float(torch.median(v)), "voiced": v.numel()}
    # the batched route measures the same frames
    assert extract_index.main(common + ["-o", str(tmp_path / "batched.pt"), "--batch-frames", "120"]) == 0
    assert torch.load(str(tmp_path / "batched.pt") + ".f0.pt") == side


def test_infer_py_auto_pitch(tmp_path):
    """`infer.py --auto-pitch -p 1` on two files of different lengths == Generator.convert(auto_pitch=True) on the same ragged batch."""
    import infer
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchRegister, attach_register, save_register
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(300, seed=2), d / "a.pt")
    save_register(d / "a.pt", PitchRegister(torch.tensor([233.0]), torch.tensor([100], dtype=torch.int32)))
    (d / "inputs").mkdir()
    waves = {"x": synth.synth_wave(1, 12000, seed=3) * 0.9, "y": synth.synth_wave(2, 16800, seed=5)[1:2] * 0.9}
    for name, w in waves.items():
        audio_io.save(str(d / "inputs" / f"{name}.wav"), w, 24000)
    common = ["-i", str(d / "inputs"), "-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "a.pt"), "-p", "1.0", "-d", DEV,
              "--seed", "3"]
    assert infer.main(common + ["-o", str(d / "out"), "--auto-pitch"]) == 0
    assert infer.main(common + ["-o", str(d / "plain")]) == 0
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), torch.device(DEV))
    tgt = attach_register(torch.load(d / "a.pt").to(DEV), d / "a.pt")
    lens = [12000, 16800]
    batch = torch.zeros(2, 16800, device=DEV)
    angle = torch.zeros(2, 961, 35, device=DEV)
    for r, name in enumerate(("x", "y")):
        wf, _sr = audio_io.load(str(d / "inputs" / f"{name}.wav"))
        batch[r, :lens[r]] = wf[0].to(DEV)
        angle[r, :, :lens[r] // 480] = infer.file_angle(gen, torch.device(DEV), 3, str(d / "inputs" / f"{name}.wav"), lens[r] // 480)[0]
    want = gen.convert(batch, tgt, 1.0, noise_angle=angle, lengths=lens, auto_pitch=True).cpu()
    for r, name in enumerate(("x", "y")):
        audio_io.save(str(d / f"want_{name}.wav"), want[r:r + 1, :lens[r]], 24000)
        got = open(d / "out" / f"{name}.wav", "rb").read()
        assert got == open(d / f"want_{name}.wav", "rb").read(), name
        assert got != open(d / "plain" / f"{name}.wav", "rb").read(), f"{name}: --auto-pitch changed nothing"
