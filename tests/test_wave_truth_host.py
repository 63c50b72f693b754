"""The truth of tests/test_gpu_tile_edges.py, proved with the oracle alone: the oracle in fp64 at the source positions ATen computes for
fp32 tensors (oracle.ref_cpu.fp32_positions), not at fp64 positions.

Plain fp64 F.interpolate moves every position by up to one fp32 ulp of `src` - 2^-8 of a sample at column 48 000 - against the fp32 arithmetic
the reference runs and the kernels restate on purpose (tinyvc_amd/csrc/small_kernels.h:lerp_coord).  Against that truth the fp32 oracle's own
worst 32-column waveform window grows with the length (5.7e-7 at T = 3, 1.1e-5 at T = 43, 7.65e-5 at T = 512) and the gate
max(3e-6, 2 x oracle) grows with it: the waveform - the only view of the last Upsample block - was held to 1.5e-4 at T = 512.  With the
positions kept in fp32 the difference is rounding alone, at most 4.4e-7 per window at every length, and the 3e-6 floor decides.

Three things are shown here, on the CPU:
  1. the restatement has ATen's positions: on fp32 input it agrees with F.interpolate within 2^-22 max|x| for every (length, factor or size)
     the FilterNet and dsp use at T = 1 .. 512, bit for bit when downsampling, and the same code with `src` rounded twice (no fma) does not;
  2. on every case of test_gpu_tile_edges.py (a) and (b) the fp32 one-thread oracle stays at or below 1.5e-6 per window on every compared
     tensor, and no tensor's gate is wider than against the plain fp64 truth;
  3. the waveform gate now refuses what it let through: the plain fp64 truth itself from T = 26 on (NOT at T <= 12, where the two
     definitions differ by less than the floor - a fact of the metric, pinned), and 1e-4 x rms on the last two columns in every case.

Every case of (a) and (b) is evaluated whole - the longest, T = 512, takes under a second per evaluation -; none is sampled or left out."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import FILTER_EDGE_LENGTHS, FLOOR, WIDE_FILM_SHAPES, _bump_trips, _gate_case, filter_edge_inputs, filter_edge_oracle, filter_named, sd64, window_errors
from oracle import ref_cpu as R

BOUND = 2.0 ** -22            # x max|x|: two fp32 roundings of the blend on either side
T_ALL = range(1, 513)


# ------------------------------------------------------------------------------------------------ 1. the positions
def _energy_frames(L):
    return (L - 64) // 64 + 1          # estimate_energy's max_pool1d(128, 64, 32)


# name -> (n_in(T), interpolate arguments(T)): every linear interpolation of filter_net, dsp and estimate_energy on T frames
INTERPS = {
    "ups.0 x2": (lambda T: T, lambda T: dict(scale_factor=2)),
    "ups.1 x3": (lambda T: 2 * T, lambda T: dict(scale_factor=3)),
    "ups.2 x4": (lambda T: 6 * T, lambda T: dict(scale_factor=4)),
    "ups.3 x4": (lambda T: 24 * T, lambda T: dict(scale_factor=4)),
    "ups.4 x5": (lambda T: 96 * T, lambda T: dict(scale_factor=5)),
    "dsp amps x480": (lambda T: T, lambda T: dict(scale_factor=480)),
    "dsp f0 size=L": (lambda T: T, lambda T: dict(size=480 * T)),
    "energy size=L": (lambda T: _energy_frames(480 * T), lambda T: dict(size=480 * T)),
    "downs.1 /5": (lambda T: 480 * T, lambda T: dict(scale_factor=1.0 / 5)),
    "downs.2 /4": (lambda T: 96 * T, lambda T: dict(scale_factor=1.0 / 4)),
    "downs.3 /4": (lambda T: 24 * T, lambda T: dict(scale_factor=1.0 / 4)),
    "downs.4 /3": (lambda T: 6 * T, lambda T: dict(scale_factor=1.0 / 3)),
}


@pytest.mark.parametrize("name", list(INTERPS))
def test_the_restatement_has_atens_positions(name):
    """fp32 in, fp32 out against F.interpolate at T = 1 .. 512: within 2^-22 max|x| at every element (the positions are the same numbers;
    what is left is the blend's own rounding), torch.equal when downsampling (lambda is 0 or 0.5: no product rounds).  Under the switch
    the fp64 path on the same numbers differs from F.interpolate on fp32 by the latter's rounding alone."""
    n_in, args = INTERPS[name]
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for T in T_ALL:
        x = torch.randn(1, 2, n_in(T), generator=g)
        want = F.interpolate(x, mode="linear", **args(T))
        got = R.interp_fp32_positions(x, **args(T))
        assert got.dtype == torch.float32 and got.shape == want.shape, f"{name} T={T}: {tuple(got.shape)} against {tuple(want.shape)}"
        if "/" in name:
            assert torch.equal(got, want), f"{name} T={T}"
        e = float((got - want).abs().max() / x.abs().max())
        worst = max(worst, e)
        assert e <= BOUND, f"{name} T={T}: {e:.2e} x max|x|"
        if T in (1, 12, 43, 512):
            with R.fp32_positions():
                got64 = R._interp(x.double(), **args(T))
            assert got64.dtype == torch.float64
            assert float((got64 - want.double()).abs().max() / x.abs().max()) <= BOUND, f"{name} T={T}: fp64 under the switch"
            assert torch.equal(R._interp(x.double(), **args(T)), F.interpolate(x.double(), mode="linear", **args(T))), "fp64 without the switch is F.interpolate"
            assert torch.equal(R._interp(x, **args(T)), want), "fp32 is F.interpolate, switch or not"
    print(f"[wave-truth] {name}: worst |restatement - F.interpolate| over T = 1 .. 512: {worst:.2e} x max|x| (bound {BOUND:.2e})")


@pytest.mark.parametrize("factor", [5, 3])
def test_positions_rounded_twice_miss_the_bound(factor):
    """The same restatement with src = fl(fl(scale (dst + 0.5)) - 0.5): one more rounding, of one ulp of src - 2^-14 of a sample at column
    2000 x factor.  It must fail the bound the fused one meets on the same input; that is what makes the bound a test of the positions."""
    x = torch.randn(2, 3, 2000, generator=torch.Generator().manual_seed(12))
    want = F.interpolate(x, scale_factor=factor, mode="linear")
    fused = float((R.interp_fp32_positions(x, scale_factor=factor) - want).abs().max() / x.abs().max())
    twice = float((R.interp_fp32_positions(x, scale_factor=factor, fused=False) - want).abs().max() / x.abs().max())
    print(f"[wave-truth] factor {factor} on randn(2, 3, 2000): fused {fused:.2e}, product rounded first {twice:.2e} x max|x|")
    assert fused <= BOUND
    assert twice > BOUND


def test_scale_conventions():
    """`size` -> float32(in) / float32(out); `scale_factor` -> float32(1 / factor) and floor(in x factor) outputs, 1 / (1 / f) included."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert R.interp_scale(7, scale_factor=480) == (3360, f32(1.0 / 480))
    assert R.interp_scale(30, scale_factor=1.0 / 3) == (10, 3.0)
    assert R.interp_scale(2400, scale_factor=1.0 / 5) == (480, 5.0)
    assert R.interp_scale(76, size=4800) == (4800, float(torch.tensor(76.0) / torch.tensor(4800.0)))
    i0, i1, w0, lam = R.lerp_positions(4, 8, 0.5)          # src = -0.25 -> 0, 0.25, 0.75, ... 3.25: both ends clamp
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25] and torch.equal(w0, 1.0 - lam)


# ------------------------------------------------------------------------------------------------ 2. and 3. the gate on the cases of the GPU file
CASES = [(1, T, None) for T in FILTER_EDGE_LENGTHS] + [(B, T, [0, 1, B // 2, B - 1]) for B, T in WIDE_FILM_SHAPES]
_CASE = {}


def _case(B, T, rows):
    """(new truth, plain fp64 truth, fp32 one-thread oracle, gates against the new truth, gates against the plain one), computed once."""
    if (B, T) not in _CASE:
        inputs = filter_edge_inputs(B, T)
        if rows is not None:
            inputs = [x[rows] for x in inputs]
        truth, ref = filter_edge_oracle(inputs)
        _e64, d64 = sd64()
        plain = filter_named(*R.filter_net(d64, *[x.double() for x in inputs], return_blocks=True))
        tag = f"host, the fp32 oracle in the GPU's place, B={B} T={T}"
        _f, gates = _gate_case(tag + ", fp32 positions", ref, truth, ref)
        _f, gates_plain = _gate_case(tag + ", plain fp64", ref, plain, ref)
        _CASE[B, T] = truth, plain, ref, gates, gates_plain
    return _CASE[B, T]


def _ids(c):
    return f"B{c[0]}-T{c[1]}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_oracle_stays_under_half_the_floor_and_no_gate_widens(case):
    """Against the fp32-position truth the fp32 oracle's worst window is at most 1.5e-6 = FLOOR / 2 on all ten tensors (measured: at most
    5.1e-7), so every gate is the floor; against the plain fp64 truth each gate is that or wider."""
    truth, plain, ref, gates, gates_plain = _case(*case)
    assert not R._FP32_POSITIONS, "the switch is off again outside its block"
    assert len(truth) == 10
    parts = []
    for name, t in truth.items():
        e = float(window_errors(ref[name], t).max())
        e_plain = float(window_errors(ref[name], plain[name]).max())
        parts.append(f"{name} {e:.2e} / {e_plain:.2e}")
        assert e <= FLOOR / 2, f"{name}: the oracle's worst window {e:.2e}"
        assert bool((gates[name] == FLOOR).all()), f"{name}: gate {gates[name].tolist()}"
        assert bool((gates[name] <= gates_plain[name]).all()), f"{name}: gate {gates[name].tolist()} against {gates_plain[name].tolist()} under the plain fp64 truth"
    print(f"[wave-truth] B={case[0]} T={case[1]}: oracle fp32 worst window vs the fp32-position truth / vs plain fp64: " + ", ".join(parts)
          + f"; wave gate {float(gates['wave'].max()):.2e} (plain fp64: {float(gates_plain['wave'].max()):.2e})")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_wave_gate_sees_a_tile_edge_error_and_exact_positions(case):
    """+ 1e-4 x rms on the last two columns of the fp32 oracle's waveform (2.5e-5 in its window) trips the gate in every case.  The plain
    fp64 truth rounded to fp32 - an interpolation MORE exact than ATen's, what a per-phase lambda table in place of lerp_coord computes -
    is refused from T = 26 on (5.5e-6 there, growing with T).  At T <= 12 it is not: 2.5e-6 at T = 12, below the floor.  That is a fact of
    the metric, pinned here; T = 25 (4.3e-6, refused as well) is logged only, the issue draws the line at 26."""
    B, T, _rows = case
    truth, plain, ref, gates, _gp = _case(*case)
    assert _bump_trips(ref, truth, gates, "wave"), "1e-4 x rms on the last two columns of the waveform must trip the window gate"
    exact = window_errors(plain["wave"].float(), truth["wave"])
    refused = bool((exact > gates["wave"][:, None]).any())
    print(f"[wave-truth] B={B} T={T}: the exact-position waveform's worst window vs the fp32-position truth {float(exact.max()):.2e}, "
          f"gate {float(gates['wave'].max()):.2e}: {'refused' if refused else 'passes'}")
    if T >= 26:
        assert refused, f"T={T}: exact positions read {float(exact.max()):.2e}, inside the gate"
        assert bool((exact.max(dim=1).values > gates["wave"]).all()), "in every row"
    elif T <= 12:
        assert not refused, f"T={T}: exact positions read {float(exact.max()):.2e}"
        assert math.isclose(float(gates["wave"].max()), FLOOR)
