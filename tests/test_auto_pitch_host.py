"""Automatic pitch (tvc_pitch_match_f32, tvc_convert_auto_f32, Generator.convert(auto_pitch=...)) without a GPU: the new symbols are declared
and exported, malformed calls are refused on the host before any engine or device work, semitones_between is the fp64 formula, the register
sidecar round-trips, and the entry scripts parse their flags."""
import math

import numpy as np
import pytest
import torch

from tinyvc_amd import _lib

NEW = ["tvc_pitch_match_f32", "tvc_workspace_bytes_auto", "tvc_convert_auto_f32", "tvc_workspace_bytes_ragged_auto", "tvc_convert_ragged_auto_f32"]


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_symbols_are_declared_and_exported(lib):
    from test_cabi import header_functions
    decl = header_functions()
    for name in NEW:
        assert name in decl, f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl[name]), name
        assert hasattr(lib, name), f"{name} is not exported"
    # argument checks come before any device work: no context, no call
    assert lib.tvc_pitch_match_f32(None, None, None, None, 1, None, 0.0, None, None, None, None, None) == -1
    assert lib.tvc_workspace_bytes_auto(None, 1, 4800, None, 1, None) == -1
    from tinyvc_amd.engine import Engine
    for name in ("pitch_match", "convert_auto", "convert_ragged_auto"):
        assert callable(getattr(Engine, name))


@pytest.fixture(scope="module")
def cpu_gen():
    """a Generator that never left the CPU: whatever reaches its engine raises TinyVCError (a RuntimeError), never ValueError"""
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_refusals_come_before_device_work(cpu_gen):
    from tinyvc_amd.module.tinyvc.feature_retrieval import Blend, PitchRegister
    wf = torch.zeros(2, 4800)
    plain = torch.zeros(1, 768, 8)
    with pytest.raises(ValueError, match="Blend"):
        cpu_gen.convert(wf, Blend([plain, plain], [0.5, 0.5]), 0.0, auto_pitch=True)
    with pytest.raises(ValueError, match="no pitch register"):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch=True)
    with_reg = torch.zeros(1, 768, 8)
    with_reg.pitch_register = PitchRegister(torch.tensor([200.0]), torch.tensor([10], dtype=torch.int32))
    with pytest.raises(ValueError, match="target 1 carries no pitch register"):
        cpu_gen.convert(wf, [with_reg, plain], 0.0, auto_pitch=True)
    with pytest.raises(ValueError, match="1 or B = 2"):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch=torch.tensor([100.0, 200.0, 300.0]))
    with pytest.raises(ValueError, match="1 shifts for a batch of 2"):
        cpu_gen.convert(wf, plain, [1.0], auto_pitch=150.0)
    with pytest.raises(ValueError, match="auto_pitch"):
        cpu_gen.convert(wf, plain, 0.0, auto_pitch="high")
    with pytest.raises(ValueError, match="return_shift"):
        cpu_gen.convert(wf, plain, 0.0, return_shift=True)
    # a well-formed call gets as far as the device - and there is none
    with pytest.raises(_lib.TinyVCError):
        cpu_gen.convert(wf, with_reg, 0.0, auto_pitch=True)


def test_resolve_auto_pitch_forms():
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchRegister, resolve_auto_pitch, target_registers
    assert resolve_auto_pitch(220, None, 3) == 220.0
    t = torch.tensor([100.0, 200.0, 300.0])
    assert resolve_auto_pitch(t, None, 3)[0] is not None and torch.equal(target_registers(resolve_auto_pitch(t, None, 3), 3, "cpu"), t)
    assert torch.equal(target_registers(resolve_auto_pitch(torch.tensor([150.0]), None, 3), 3, "cpu"), torch.full((3,), 150.0))
    assert torch.equal(target_registers(180.0, 2, "cpu"), torch.full((2,), 180.0))
    tg = [torch.zeros(1, 768, 4) for _ in range(2)]
    for i, x in enumerate(tg):
        x.pitch_register = PitchRegister(torch.tensor([100.0 + i]), torch.tensor([5], dtype=torch.int32))
    assert torch.equal(target_registers(resolve_auto_pitch(True, tg, 2), 2, "cpu"), torch.tensor([100.0, 101.0]))
    with pytest.raises(ValueError, match="2 target registers for a batch of 3"):
        resolve_auto_pitch(True, tg, 3)


def test_semitones_between_is_the_fp64_formula():
    from tinyvc_amd.module.tinyvc.feature_retrieval import semitones_between
    rng = np.random.default_rng(3)
    src = np.exp(rng.uniform(np.log(20.1), np.log(3000.0), 64))
    tgt = np.exp(rng.uniform(np.log(20.1), np.log(3000.0), 64))
    want = 12.0 * np.log2(tgt / src)
    got = semitones_between(src.tolist(), tgt.tolist())
    assert np.allclose(np.array(got), want, rtol=0, atol=1e-12)      # two fp64 evaluations of one expression: a few ulps of values below 90
    assert semitones_between(110.0, 220.0) == 12.0 and semitones_between(220.0, 110.0) == -12.0 and semitones_between(123.0, 123.0) == 0.0
    assert semitones_between(torch.tensor([110.0, 220.0]), 220.0) == [12.0, 0.0]
    # no register on either side: no automatic shift, as on the device
    assert semitones_between(0.0, 220.0) == 0.0 and semitones_between(110.0, 0.0) == 0.0 and semitones_between(110.0, math.nan) == 0.0
    with pytest.raises(ValueError):
        semitones_between([1.0, 2.0], [1.0])


def test_sidecar_is_written_and_loaded(tmp_path):
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchRegister, attach_register, save_register, sidecar_path
    path = tmp_path / "index.pt"
    index = torch.zeros(1, 768, 4)
    torch.save(index, path)
    before = open(path, "rb").read()
    assert getattr(attach_register(torch.load(path), path), "pitch_register", None) is None      # no sidecar: nothing attached
    save_register(path, PitchRegister(torch.tensor([187.25]), torch.tensor([4321], dtype=torch.int32)))
    assert sidecar_path(path) == str(path) + ".f0.pt" and open(path, "rb").read() == before
    d = torch.load(sidecar_path(path))
    assert d == {"median_hz": 187.25, "voiced": 4321}
    reg = attach_register(torch.load(path), path).pitch_register
    assert reg.median_hz.dtype == torch.float32 and reg.median_hz.tolist() == [187.25] and reg.voiced.tolist() == [4321]


def test_entry_scripts_parse_their_flags():
    import infer
    import infer_streaming
    assert infer.build_parser().parse_args([]).auto_pitch is False
    a = infer.build_parser().parse_args(["--auto-pitch", "-p", "2.5"])
    assert a.auto_pitch is True and a.pitch_shift == 2.5
    assert infer_streaming.build_parser().parse_args([]).auto_pitch_from is None
    assert infer_streaming.build_parser().parse_args(["--auto-pitch-from", "calib.wav"]).auto_pitch_from == "calib.wav"
