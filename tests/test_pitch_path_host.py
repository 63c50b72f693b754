"""The pitch path without a GPU, on the numpy restatement the GPU tests hold the kernel to (helpers_pitch_path): the banded shortcut the
kernel computes equals the full 512 x 512 definition bit for bit - paths, back-pointers, scores - on logits and costs quantised to
multiples of 0.25 (all arithmetic exact, equal values everywhere) and on Gaussian logits; zero costs are the per-frame lowest argmax; a
planted one-frame octave flip stays on the ridge where the per-frame top-4 decode leaves it; a planted one-frame class-0 drop-out inside a
voiced run is bridged while its margin is below 2 * voicing.  Then what is refused on the host - PitchPath's settings, the new symbols in
header, binding and library - and the entry scripts' flags.  The defaults are guesses: nobody has listened."""
import math
import types

import numpy as np
import pytest
import torch

import helpers_pitch_path as H
from helpers import decode_lower_id_first
from tinyvc_amd import _lib
from tinyvc_amd.engine import pitch_class_table
from tinyvc_amd.module.tinyvc.feature_retrieval import PitchPath, f0_keywords, resolve_f0_estimation

F = np.float32
INF = math.inf
LENGTHS = [1, 2, 3, 28]
# (step, band, jump, voicing): multiples of 0.25, jump == band * step exactly (the edge of the condition), above it, and +inf
QUANTISED_COSTS = [(0.25, 3, 0.75, 0.5), (0.25, 3, 1.0, 0.75), (0.5, 12, 6.0, 0.25), (0.0, 32, 0.0, 0.0), (0.25, 0, 0.0, 1.0), (0.25, 32, 8.0, 0.5),
                   (0.5, 2, INF, 0.5), (0.25, 4, 1.0, INF), (0.75, 1, 0.75, 0.0)]


def same(a, b):
    (pa, ba, sa), (pb, bb, sb) = a, b
    return np.array_equal(pa, pb) and np.array_equal(ba, bb) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("costs", QUANTISED_COSTS)
def test_banded_equals_full_on_quantised_logits(T, costs):
    s = H.Settings(*costs, 0)
    for seed in range(2):
        x = H.quantised(T, 100 * T + seed, levels=5 + 4 * seed)
        full, banded = H.viterbi_full(x, s), H.viterbi_banded(x, s)
        assert same(full, banded), (T, costs, seed)
    if T == 28 and costs[2] < INF:      # the inputs do hold equal candidates: some back-pointer is decided by the lowest-class rule alone
        e, cost = H.emission(x), H.cost_matrix(s)
        sc = (e[:, 0] - e[:, 0].max()).astype(F)
        cand = (sc[:, None] - cost).astype(F)
        assert ((cand == cand.max(axis=0)).sum(axis=0) > 1).any()


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("settings", [H.DEFAULT, H.Settings(0.3, 5, 1.7, 0.9, 0), H.Settings(0.05, 32, 1.6000001, 2.5, 0), H.Settings(0.5, 12, INF, INF, 0)])
def test_banded_equals_full_on_gaussian_logits(T, settings):
    x = H.gaussian(T, 7 * T + 1)
    assert same(H.viterbi_full(x, settings), H.viterbi_banded(x, settings))


def test_special_values_stay_finite_and_agree():
    x = H.special_columns(28, 5)
    full, banded = H.viterbi_full(x, H.DEFAULT), H.viterbi_banded(x, H.DEFAULT)
    assert same(full, banded) and np.isfinite(full[2]).all() and full[2].max() == 0


@pytest.mark.parametrize("make", [H.gaussian, H.quantised])
def test_zero_costs_are_the_per_frame_lowest_argmax(make):
    x = make(28, 3)
    for form in (H.viterbi_full, H.viterbi_banded):
        path, _bp, _sc = form(x, H.Settings(0.0, 12, 0.0, 0.0, 0))
        assert np.array_equal(path, np.argmax(x, axis=0))


def test_planted_octave_flip_stays_on_the_ridge():
    """class c + 48 is higher by less than `jump` on one frame: the path pays nothing to stay, 2 * jump to leave and return"""
    c, t, T = 150, 13, 28
    freq = pitch_class_table().numpy()
    for margin in (0.5, 6.0, 11.5):
        x = H.planted_flip(T, c, t, margin)
        path, _bp, _sc = H.viterbi_banded(x, H.DEFAULT)
        assert (path == c).all(), margin
        assert np.array_equal(path, H.viterbi_full(x, H.DEFAULT)[0])
        f0 = H.frequency(x, path, 0, freq)
        assert (f0 == freq[c]).all()
        # the per-frame decode leaves the ridge on that frame: its top class there is the octave, and its f0 lies above the ridge's
        top4_f0, _raw, ids, _tie = decode_lower_id_first(torch.from_numpy(x)[None])
        assert int(ids[0, 0, t]) == c + 48 and float(top4_f0[0, 0, t]) > 1.2 * freq[c]
        assert abs(float(top4_f0[0, 0, t - 1]) - freq[c]) < 0.02 * freq[c]
    far = H.planted_flip(T, c, t, 2 * 12.0 + 1.0)      # above 2 * jump the detour pays
    assert H.viterbi_banded(far, H.DEFAULT)[0][t] == c + 48


def test_planted_dropout_is_bridged_below_twice_voicing():
    c, t, T = 200, 9, 28
    for margin in (0.25, 3.0, 5.75):
        x = H.planted_dropout(T, c, t, margin)
        path = H.viterbi_banded(x, H.DEFAULT)[0]
        assert (path == c).all(), margin
        assert np.argmax(x[:, t]) == 0      # frame by frame it is unvoiced
    assert H.viterbi_banded(H.planted_dropout(T, c, t, 6.5), H.DEFAULT)[0][t] == 0      # above 2 * voicing the drop-out is believed
    assert H.viterbi_banded(H.planted_dropout(T, c, t, 100.0), H.DEFAULT._replace(voicing=INF))[0][t] == c      # voicing = inf never changes


def test_frequency_refine_zero_is_the_class_frequency_and_refine_is_bounded():
    freq = pitch_class_table().numpy()
    x = H.gaussian(28, 11)
    path = H.viterbi_banded(x, H.DEFAULT)[0]
    path[3], path[5], path[7] = 0, 1, 511
    f0 = H.frequency(x, path, 0, freq)
    assert np.array_equal(f0, np.where(path == 0, F(0), freq[path]))
    for r in (1, 2, 4):
        got, truth = H.frequency(x, path, r, freq).astype(np.float64), H.frequency64(x, path, r, freq)
        assert (np.abs(got - truth) <= H.f0_bound(r) * truth).all() and (got[path == 0] == 0).all()


# ---- refusals and plumbing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(jump=5.9), dict(band=33), dict(band=-1), dict(refine=5), dict(refine=-1), dict(step=float("nan")),
                                dict(jump=float("nan")), dict(voicing=float("nan")), dict(step=-0.5), dict(step=INF), dict(voicing=-1.0),
                                dict(band=12.5), dict(refine=True), dict(step="0.5")])
def test_settings_are_refused_on_the_host(kw):
    with pytest.raises(ValueError, match="f0_estimation"):
        PitchPath(**kw)


def test_settings_defaults_and_forms():
    p = PitchPath()
    assert p.params() == (0.5, 12, 12.0, 3.0, 2) == tuple(H.DEFAULT)
    assert PitchPath(jump=INF, voicing=INF).params()[2:4] == (INF, INF)
    assert PitchPath(step=0.5, band=12, jump=6.0).jump == 6.0      # jump == band * step is legal
    s = p.settings()
    assert isinstance(s, _lib.PitchPathSettings) and (s.step, s.band, s.jump, s.voicing, s.refine) == p.params()
    assert resolve_f0_estimation("viterbi").params() == p.params() and resolve_f0_estimation(p) is p
    for other in ("default", "harvest", "fcpe", "dio", None, 3):
        assert resolve_f0_estimation(other) is None


def test_symbols_in_header_binding_and_library():
    from test_cabi import header_functions
    from tinyvc_amd import build
    build.build(verbose=False)
    lib, decl = _lib.load_library(), header_functions()
    for name in ("tvc_pitch_path_f32", "tvc_workspace_bytes_pitch_path", "tvc_convert_path_f32", "tvc_convert_ragged_path_f32", "tvc_workspace_bytes_path",
                 "tvc_workspace_bytes_ragged_path"):
        assert name in decl and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(decl["tvc_convert_path_f32"]) == len(decl["tvc_convert_protect_f32"]) + 1
    assert len(decl["tvc_convert_ragged_path_f32"]) == len(decl["tvc_convert_ragged_protect_f32"]) + 1
    assert lib.tvc_pitch_path_f32(None, None, None, None, None, 0, 0, None, 0.0, None, None, None, None, None, None, 0) == -1      # null ctx


def test_entry_script_flags(capsys):
    import infer
    import infer_streaming
    for m, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        args = m.build_parser().parse_args([])
        assert args.f0_estimation == "default" and f0_keywords(args, name) == "default"
        args = m.build_parser().parse_args(["-f0-est", "viterbi"])
        assert f0_keywords(args, name).params() == PitchPath().params()
        args = m.build_parser().parse_args(["-f0-est", "viterbi", "--f0-step", "0.25", "--f0-band", "8", "--f0-jump", "4", "--f0-voicing", "2", "--f0-refine", "0"])
        assert f0_keywords(args, name).params() == (0.25, 8, 4.0, 2.0, 0)
        assert "nobody has listened" in capsys.readouterr().out
        with pytest.raises(SystemExit, match="jump"):
            f0_keywords(m.build_parser().parse_args(["-f0-est", "viterbi", "--f0-jump", "1"]), name)
        with pytest.raises(SystemExit, match="belongs to -f0-est viterbi"):
            f0_keywords(m.build_parser().parse_args(["--f0-band", "8"]), name)
        assert "--f0-voicing" in m.build_parser().format_help()
    assert f0_keywords(infer.build_parser().parse_args(["-f0-est", "harvest"]), "infer.py") == "harvest"      # ignored, as in the reference
    with pytest.raises(SystemExit):
        infer_streaming.build_parser().parse_args(["-f0-est", "crepe"])      # the streaming script lists its names
    assert f0_keywords(types.SimpleNamespace(f0_estimation="dio"), "x") == "dio"
