"""The pitch path's carry without a GPU, on the numpy restatement the GPU tests hold the kernel to (helpers_pitch_carry on
helpers_pitch_path).  The prefix property: windows of T frames advancing by h over ONE logits tensor, each started from the carry of the one
before, give - by value - the scores, back-pointers and path of helpers_pitch_path's decode of the whole prefix.  A prior of zeros is no
prior; every carry has maximum exactly 0; the sanitising rule; infinite costs.  Then the host's refusals (PitchCarry, the streams' f0_carry,
Generator.convert's carry, the scripts' --f0-carry), the state table, and the new symbols in header, binding and library."""
import math
import types

import numpy as np
import pytest
import torch

import helpers_pitch_carry as C
import helpers_pitch_path as H
from tinyvc_amd import _lib, stream_state
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchCarry, PitchPath, check_f0_carry, f0_carry_keywords

F = np.float32
INF = math.inf
SHAPES = [(12, 4), (5, 4), (6, 1), (28, 4)]      # (T, h)
NWIN = 6
INPUTS = {"gaussian": H.gaussian, "quantised": H.quantised, "special": H.special_columns}


def _prefix_check(x, s, T, h, what):
    wins = C.windows(x, s, T, h, NWIN)
    for n, (path, bp, sc, carry) in enumerate(wins):
        end = n * h + T
        want_path, want_bp, want_sc = H.viterbi_banded(x[:, :end], s)
        assert np.array_equal(sc, want_sc), f"{what} window {n}: scores"
        assert np.array_equal(bp[1:], want_bp[end - T + 1:end]), f"{what} window {n}: back-pointers"
        assert np.array_equal(path, want_path[end - T:]), f"{what} window {n}: path"
        assert carry.max() == 0 and not np.isnan(carry).any() and (carry <= 0).all(), f"{what} window {n}: carry"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}h{s[1]}")
@pytest.mark.parametrize("kind", list(INPUTS))
def test_windows_equal_the_decode_of_the_whole_prefix(kind, shape):
    T, h = shape
    x = INPUTS[kind]((NWIN - 1) * h + T, 31 * T + h)
    _prefix_check(x, H.DEFAULT, T, h, f"{kind} {shape}")


@pytest.mark.parametrize("settings", [H.Settings(0.5, 12, INF, 3.0, 2), H.Settings(0.3, 5, 1.7, INF, 1), H.Settings(0.5, 12, INF, INF, 0)])
def test_infinite_costs(settings):
    x = H.gaussian(5 * 4 + 12, 77)
    _prefix_check(x, settings, 12, 4, str(settings))
    # a carry is -inf only under infinite costs: from a state that knows class 300 alone, class 0 is out of reach at voicing = inf and the
    # classes beyond the band at jump = inf; under finite costs every class has a finite route
    only = np.full(512, -INF, F)
    only[300] = 0
    carry = C.viterbi_carried(x[:, :12], settings, only, 1)[3]
    assert np.isneginf(carry[0]) == (settings.voicing == INF) and np.isneginf(carry[400]) == (settings.jump == INF) and carry[300] == 0
    assert np.isfinite(C.viterbi_carried(x[:, :12], H.DEFAULT, only, 1)[3]).all()


def test_zero_prior_is_no_prior():
    for x in (H.gaussian(12, 3), H.quantised(12, 4), H.special_columns(12, 5)):
        a, b = C.viterbi_carried(x, H.DEFAULT, None, 4), C.viterbi_carried(x, H.DEFAULT, np.zeros(512, F), 4)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        full = H.viterbi_full(x, H.DEFAULT)
        assert all(np.array_equal(p, q) for p, q in zip(a[:3], full))


def test_the_sanitising_rule():
    r = np.random.default_rng(9)
    good = -np.abs(r.standard_normal(512)).astype(F) * 5
    good[7] = -INF
    dirty = good.copy()
    dirty[[1, 2, 3, 4]] = [np.nan, INF, 3.5, F(1e-30)]
    clean = good.copy()
    clean[[1, 2, 3, 4]] = 0
    assert np.array_equal(C.sanitise(dirty), clean) and np.array_equal(C.sanitise(good), good)
    assert np.array_equal(C.sanitise(np.full(512, -INF, F)), np.zeros(512, F))                       # -inf throughout: a reset
    mixed = np.full(512, -INF, F)
    mixed[5] = np.nan                                                                              # NaN counts as 0 BEFORE the all -inf rule
    assert C.sanitise(mixed)[5] == 0 and np.isneginf(C.sanitise(mixed)).sum() == 511
    x = H.gaussian(12, 6)
    for state in (np.full(512, np.nan, F), np.full(512, INF, F), np.full(512, 2.0, F), np.full(512, -INF, F)):
        a, b = C.viterbi_carried(x, H.DEFAULT, state, 4), C.viterbi_carried(x, H.DEFAULT, None, 4)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # a prior does steer the decode: everything but class 300 far behind puts frame 0 there
    steer = np.full(512, -50.0, F)
    steer[300] = 0
    assert C.viterbi_carried(x, H.DEFAULT, steer, 4)[0][0] == 300 and C.viterbi_carried(x, H.DEFAULT, None, 4)[0][0] != 300
    sc = C.viterbi_carried(x, H.DEFAULT, dirty, 4)[2]
    assert sc.max() == 0 and not np.isnan(sc).any()


@pytest.mark.parametrize("margin,gap", [(0.25, 9.0), (0.5, 6.0), (0.75, 3.0)])
def test_planted_octave_the_carried_window_stays_where_the_uncarried_one_leaves(margin, gap):
    x = C.planted_octave(margin)
    wins = C.windows(x, H.DEFAULT, 12, 4, 3)
    path, _bp, sc, _carry = wins[2]                                 # frames 8 .. 19, carried
    assert (path == 200).all()
    assert sc[200] == 0 and sc[248] == F(-gap)
    alone = C.viterbi_carried(x[:, 8:20], H.DEFAULT)[0]             # the same frames from a flat start
    assert (alone == 248).all()


# ---- the state table ---------------------------------------------------------------------------------------------------------------------
def test_carry_state_allocate_reset_addresses():
    assert [tuple(f) for f in stream_state.CARRY_STATE] == [("scores", torch.float32, 512, 0.0)]
    c = PitchCarry(3, 4, device="cpu")
    assert c.params() == (4,) and c.scores.shape == (3, 512) and c.scores.dtype == torch.float32 and not c.scores.any()
    where = stream_state.addresses(c, stream_state.CARRY_STATE)
    c.scores.fill_(-2.0)
    c.reset([1])
    assert (c.scores[1] == 0).all() and (c.scores[[0, 2]] == -2.0).all()
    c.reset()
    assert not c.scores.any() and stream_state.addresses(c, stream_state.CARRY_STATE) == where      # in place: never rebound
    assert stream_state.checked(c, stream_state.CARRY_STATE, 3, torch.device("cpu"), "carry.")[0] is c.scores
    c.scores = c.scores[:, :256]
    with pytest.raises(ValueError, match="carry.scores"):
        stream_state.checked(c, stream_state.CARRY_STATE, 3, torch.device("cpu"), "carry.")


# ---- refusals on the host -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(0, 4), (2, 0), (2, -1), (True, 4), (2, 4.0), (2, "4")])
def test_pitch_carry_arguments_are_refused(args):
    with pytest.raises(ValueError, match="PitchCarry"):
        PitchCarry(*args, device="cpu")


def test_f0_carry_of_a_stream_is_refused_before_anything_is_allocated():
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    assert check_f0_carry(False, "default", 1000, 2) is None and check_f0_carry(None, "viterbi", 1920, 2) is None
    assert check_f0_carry(True, "viterbi", 1920, 2) is True and check_f0_carry(True, PitchPath(), 480, 1) is True
    fits = PitchCarry(2, 4, device="cpu")
    assert check_f0_carry(fits, "viterbi", 1920, 2) is fits
    for bad, est, block, match in ((True, "default", 1920, "needs f0_estimation"), (True, "harvest", 1920, "needs f0_estimation"),
                                   (True, "viterbi", 2000, "480"), (fits, "viterbi", 960, "a carry of 2 streams advancing 4"),
                                   (PitchCarry(3, 4, device="cpu"), "viterbi", 1920, "a carry of 3 streams"), ("yes", "viterbi", 1920, "f0_carry")):
        with pytest.raises(ValueError, match=match):
            check_f0_carry(bad, est, block, 2)
    # the constructors refuse before they touch the generator (None here) or a device
    with pytest.raises(ValueError, match="needs f0_estimation"):
        BatchedStreamInfer(None, n_streams=2, f0_carry=True)
    with pytest.raises(ValueError, match="480"):
        BatchedStreamInfer(None, n_streams=2, block_size=2000, extra_size=4000, last_delay_size=3840, f0_estimation="viterbi", f0_carry=True)
    with pytest.raises(ValueError, match="needs f0_estimation"):
        StreamInfer(types.SimpleNamespace(_module_device=lambda: torch.device("cpu")), f0_carry=True)


def test_convert_refuses_a_carry_it_cannot_take():
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    gen = Generator(Encoder(), Decoder())
    wf, tgt = torch.zeros(2, 28 * 480), torch.zeros(1, 768, 16)
    carry = PitchCarry(2, 4, device="cpu")
    with pytest.raises(ValueError, match="carry needs f0_estimation"):
        gen.convert(wf, tgt, 0.0, carry=carry)
    with pytest.raises(ValueError, match="carry with lengths"):
        gen.convert(wf, tgt, 0.0, f0_estimation="viterbi", carry=carry, lengths=[9600, 9600])
    with pytest.raises(ValueError, match="a carry of 3 streams"):
        gen.convert(wf, tgt, 0.0, f0_estimation="viterbi", carry=PitchCarry(3, 4, device="cpu"))
    with pytest.raises(ValueError, match="hop_frames = 28"):
        gen.convert(wf, tgt, 0.0, f0_estimation=PitchPath(), carry=PitchCarry(2, 28, device="cpu"))


def test_symbols_in_header_binding_and_library():
    from test_cabi import header_functions
    from tinyvc_amd import build
    build.build(verbose=False)
    lib, decl = _lib.load_library(), header_functions()
    for name in ("tvc_pitch_path_carry_f32", "tvc_convert_carry_f32"):
        assert name in decl and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(decl["tvc_pitch_path_carry_f32"]) == len(decl["tvc_pitch_path_f32"]) + 3
    assert len(decl["tvc_convert_carry_f32"]) == len(decl["tvc_convert_path_f32"]) + 2
    assert lib.tvc_pitch_path_carry_f32(None, None, None, None, None, 0, 0, None, 0, None, None, 0.0, None, None, None, None, None, None, 0) == -1
    assert lib.tvc_convert_carry_f32(None, None, None, None, None, 0, None, None, None, None, 0, None, None, 0, 0, 0, 0, 0.0, None, None, None, 0.0, None,
                                     None, None, 0, None, 0, 0, None, 0) == -1


def test_entry_script_flags(capsys):
    import infer
    import infer_streaming
    for m, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        assert f0_carry_keywords(m.build_parser().parse_args([]), name) == {}
        assert f0_carry_keywords(m.build_parser().parse_args(["-f0-est", "viterbi", "--f0-carry"]), name) == {"f0_carry": True}
        assert "nobody has listened" in capsys.readouterr().out
        with pytest.raises(SystemExit, match="--f0-carry belongs to -f0-est viterbi"):
            f0_carry_keywords(m.build_parser().parse_args(["--f0-carry"]), name)
        assert "--f0-carry" in m.build_parser().format_help()
    assert "f0_carry" in infer.convert_chunked.__doc__
