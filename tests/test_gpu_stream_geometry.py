"""The streaming tail at a chosen geometry (tvc_sola_geom_f32 through Engine.sola(crossfade=, search=, delay=)) and streams built on it
(BatchedStreamInfer(crossfade_size=, sola_search_size=, last_delay_size=), infer_streaming.py --crossfade --sola-search --lookahead), in the
manner of tests/test_gpu_sola.py, whose helpers this file reuses where they do not assume 1920 / 1920 / 3840.

Truth is oracle.ref_cpu.sola_tail, which takes `search` and `delay` and reads `cross` off the buffer's length: the fp64 copy decides lags,
the fp32 copy (one thread) is the bit-for-bit reference of everything that is not a sum.  Its `y[... : -delay]` slicing cannot express
delay = 0: the truth for that case is delay = 1 on y with one poison sample appended (which no slice reaches).  A lag is compared only
where fp32 can decide it: the fp64 gap between the best and the second-best correlation is asserted, never skipped, to exceed
2 * cross * 2^-24 * ||sola||; the seeds were chosen on the CPU so that it holds for every case.

Every lag check runs in both launch layouts: a handful of rows (split search: sola_corr_kernel, 8 lag groups of ceil((search + 1) / 8)
lags) and 1025 rows cycling through the cases (the one-workgroup search inside sola_kernel).  The whole file takes a few seconds."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import oracle_one_thread, rms, state_dicts
from oracle import ref_cpu as R
from test_gpu_parity import _log
from test_gpu_sola import S_ONE_WG, first_diff, gap64, layouts, same_bits
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (cross, search, delay, block)
MINIMAL = (4, 0, 0, 1)                    # everything minimal, one lag, block < cross
README = (240, 240, 480, 480)             # README.md's example
ONE_PER_GROUP = (480, 7, 1, 100)          # 8 lags: one per lag group
EMPTY_GROUPS = (480, 5, 0, 480)           # 6 lags: two groups start past the last lag; block == cross
NEAR_CAPS = (1916, 1919, 3, 5000)         # near the caps, nothing round, block > cross
FULL_SEARCH = (960, 1920, 3840, 200)      # block < cross with a full search
GEOMS = [MINIMAL, README, ONE_PER_GROUP, EMPTY_GROUPS, NEAR_CAPS, FULL_SEARCH]
LY_EXTRA = [0, 333]                       # Ly above the minimum; 333: rows that do not start on a multiple of 4 floats
POISON = 1e30


def gid(g):
    return "-".join(str(v) for v in g)


def fade(cross):
    """StreamState.fade_in at `cross`: the first cross entries of the reference's expression (arange's float step gives cross + 1 for some)"""
    return torch.sin(math.pi * torch.arange(0, 1, 1 / cross)[:cross] / 2) ** 2


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


# ----------------------------------------------------------------------------------------------- the only device access of the tail tests
def gpu_tail(eng, y, sola, geom, pv=False):
    """Engine.sola at `geom` on host tensors y [S, Ly], sola [S, cross] -> (out [S, block], new buffer [S, cross], shift [S]) on the host."""
    cross, search, delay, block = geom
    buf = sola.to(DEV).clone()
    out, shift = eng.sola(y.to(DEV), buf, fade(cross).to(DEV), block, use_phase_vocoder=pv, want_shift=True, crossfade=cross, search=search, delay=delay)
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu(), shift.cpu().long()


# ----------------------------------------------------------------------------------------------- references
def min_ly(geom):
    return sum(geom)


def temp_wav(y, geom):
    """The window of y the tail works on (stream.py:74), [.., block + cross + search]: a view."""
    cross, search, delay, block = geom
    n = y.shape[-1]
    return y[..., n - block - cross - search - delay:n - delay]


def oracle(y, sola, geom, pv=False, dtype=torch.float32):
    """R.sola_tail per stream -> lists of out, new buffer, shift, corr.  delay = 0: delay = 1 on y with one poison sample appended."""
    cross, search, delay, block = geom
    if delay == 0:
        y = torch.cat([y, torch.full((y.shape[0], 1), POISON, dtype=y.dtype)], dim=1)
        delay = 1
    res = [R.sola_tail(y[s].to(dtype), sola[s].to(dtype), fade(cross).to(dtype), block, pv, search=search, delay=delay) for s in range(y.shape[0])]
    return [list(c) for c in zip(*res)]


def gap(corr):
    """gap64 where there is a second lag; a search of one lag is decided"""
    return gap64(corr) if corr.numel() > 1 else (0, math.inf)


def decidable_bound(sola, cross):
    """What a cross-term fp32 sum can move a correlation by: |nom| / ||window|| <= ||sola||, each of the two compared values within
    cross * 2^-24 of its own."""
    return 2 * cross * 2.0 ** -24 * float(sola.double().norm())


def np_tail(y, sola, shift, geom):
    """The sin^2 tail at a given lag in plain numpy float32: products and the sum rounded one by one, everything else a copy."""
    cross, search, delay, block = geom
    tw = temp_wav(y, geom).numpy()
    fi = fade(cross).numpy()
    seg = tw[shift:shift + block + cross]
    head = seg[:cross] * fi + sola.numpy() * (np.float32(1) - fi)
    assert head.dtype == np.float32
    temp = np.concatenate([head, seg[cross:]])
    return temp[:block], temp[block:], head


def planted(geom, extra, lags, seed):
    """white noise rows with 0.7 x the buffer planted at lags[s] of row s's window"""
    cross, search, delay, block = geom
    g = torch.Generator().manual_seed(seed)
    y = 0.1 * torch.randn(len(lags), min_ly(geom) + extra, generator=g)
    sola = 0.1 * torch.randn(len(lags), cross, generator=g)
    tw = temp_wav(y, geom)
    for s, lag in enumerate(lags):
        tw[s, lag:lag + cross] = 0.7 * sola[s]
    return y, sola


def check_both_layouts(eng, geom, y, sola, lags, what):
    """lags, blocks and next buffers of both layouts against the fp32 oracle (one thread) and plain numpy, to the bit"""
    cross, search, delay, block = geom
    n = len(lags)
    with oracle_one_thread():
        ref_out, ref_buf, ref_shift, _c = oracle(y, sola, geom)
    assert ref_shift == lags, f"{what}: the fp32 oracle's lags {ref_shift}"
    e_out = torch.stack([torch.from_numpy(np_tail(y[c], sola[c], lags[c], geom)[0]) for c in range(n)])
    e_buf = torch.stack([torch.from_numpy(np_tail(y[c], sola[c], lags[c], geom)[1]) for c in range(n)])
    assert same_bits(e_out, torch.stack(ref_out)) and same_bits(e_buf, torch.stack(ref_buf)), f"{what}: numpy and the fp32 oracle differ"
    for name, rows in layouts(n):
        # (one-wg: each cycle through the cases is scaled by another power of two, which scales every product and sum of the tail
        # exactly - no value comes near the subnormals - so the rows differ and the oracle's rows still apply)
        scale = torch.tensor([2.0 ** -(r // n % 4) for r in range(len(rows))])[:, None]
        out, buf, shift = gpu_tail(eng, y[rows] * scale, sola[rows] * scale, geom)
        want = [lags[c] for c in rows]
        bad = [(r, int(shift[r]), want[r]) for r in range(len(rows)) if int(shift[r]) != want[r]]
        assert not bad, f"{what} {name}: {len(bad)} lags differ, (stream, got, want): {bad[:6]}"
        assert same_bits(out, e_out[rows] * scale), f"{what} {name}: out: {first_diff(out, e_out[rows] * scale)}"
        assert same_bits(buf, e_buf[rows] * scale), f"{what} {name}: buffer: {first_diff(buf, e_buf[rows] * scale)}"
    if block < cross:      # the next buffer: the rest of the cross-faded head, then raw samples behind it
        for c in range(n):
            head = np_tail(y[c], sola[c], lags[c], geom)[2]
            tw = temp_wav(y[c], geom)
            assert same_bits(e_buf[c, :cross - block], head[block:]) and same_bits(e_buf[c, cross - block:], tw[lags[c] + cross:lags[c] + cross + block])


# ----------------------------------------------------------------------------------------------- every geometry, both Ly, both layouts
def random_lags(geom, n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, geom[1] + 1, n)]


@pytest.mark.parametrize("extra", LY_EXTRA)
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_every_geometry_to_the_bit(eng, geom, extra):
    """Six rows per geometry, the buffer planted somewhere in the search range (at its two ends in rows 0 and 1): the lag is the fp64
    oracle's, where fp32 can decide it - asserted for every row -, and the block and the next buffer are the fp32 oracle's to the bit."""
    cross, search, delay, block = geom
    seed = 4000 + cross + extra
    lags = [0, search] + random_lags(geom, 4, seed)
    y, sola = planted(geom, extra, lags, seed)
    assert y.shape[1] == min_ly(geom) + extra
    _o, _b, shift64, corr64 = oracle(y, sola, geom, dtype=torch.float64)
    for c, lag in enumerate(lags):
        best, g = gap(corr64[c])
        assert corr64[c].numel() == search + 1 and shift64[c] == lag and (best == lag or search == 0), f"precondition: row {c}: fp64 lag {shift64[c]}, planted {lag}"
        assert g > decidable_bound(sola[c], cross), f"precondition: row {c} not decidable: gap {g:.3e} <= {decidable_bound(sola[c], cross):.3e}"
    check_both_layouts(eng, geom, y, sola, lags, f"{gid(geom)} Ly +{extra}")


# ----------------------------------------------------------------------------------------------- planted lags at the group seams
def seam_lags(search):
    lpg = -(-(search + 1) // 8)      # the run-time LPG
    return [0, lpg - 1, lpg, 2 * lpg - 1, 2 * lpg, 7 * lpg - 1, 7 * lpg, search]


@pytest.mark.parametrize("geom", [README, NEAR_CAPS], ids=gid)
def test_planted_lags_at_the_seams_of_the_run_time_lag_groups(eng, geom):
    cross, search, delay, block = geom
    lags = seam_lags(search)
    if search == 240:
        assert lags == [0, 30, 31, 61, 62, 216, 217, 240]
    else:
        assert lags == [0, 239, 240, 479, 480, 1679, 1680, 1919]
    y, sola = planted(geom, 333, lags, seed=5000 + search)
    _o, _b, _s, corr64 = oracle(y, sola, geom, dtype=torch.float64)
    for c, lag in enumerate(lags):
        best, g = gap(corr64[c])
        assert best == lag and g >= 0.5, f"precondition: planted lag {lag} is not decisive in fp64 (best {best}, gap {g:.3f})"
    check_both_layouts(eng, geom, y, sola, lags, f"seams {gid(geom)}")


# ----------------------------------------------------------------------------------------------- exact ties, NaN
TIES = {README: [(31, 0), (31, 30), (100, 37), (7, 3)], FULL_SEARCH: [(241, 0), (241, 240), (256, 5), (100, 99)]}      # (period, phase)


@pytest.mark.parametrize("geom", list(TIES), ids=gid)
def test_exact_ties_keep_the_lowest_lag(eng, geom):
    """y exactly periodic in fp32, the buffer one window of it: every lag = phase (mod period) sees the same window, the same sums in the
    same order, the same correlation; the first maximum is the reference's rule.  The periods tie the first or the last lag of every group
    of the split search (31 at search 240, 241 at 1920) and the lags of ONE thread of the one-workgroup loop (256)."""
    cross, search, delay, block = geom
    ties = TIES[geom]
    g = torch.Generator().manual_seed(78)
    y = torch.zeros(len(ties), min_ly(geom) + 5)
    sola = torch.zeros(len(ties), cross)
    for c, (P, phi) in enumerate(ties):
        pat = 0.1 * torch.randn(P, generator=g)
        temp_wav(y, geom)[c] = pat[torch.arange(block + cross + search) % P]
        sola[c] = pat[(phi + torch.arange(cross)) % P]
    _o, _b, shift64, corr64 = oracle(y, sola, geom, dtype=torch.float64)
    for c, (P, phi) in enumerate(ties):
        at_max = (corr64[c] == corr64[c].max()).nonzero().flatten().tolist()
        assert at_max == list(range(phi, search + 1, P)) and len(at_max) > 1 and shift64[c] == phi, f"precondition: period {P} phase {phi}: fp64 maxima at {at_max}"
    for name, rows in layouts(len(ties)):
        out, buf, shift = gpu_tail(eng, y[rows], sola[rows], geom)
        assert shift.tolist() == [ties[c][1] for c in rows], f"{name}: {shift.tolist()[:12]} ... for (period, phase) {ties}"
        for r, c in list(enumerate(rows))[:2 * len(ties)]:
            e_out, e_buf, _h = np_tail(y[c], sola[c], ties[c][1], geom)
            assert same_bits(out[r], e_out) and same_bits(buf[r], e_buf), f"{name} stream {r}"


@pytest.mark.parametrize("S", [3, S_ONE_WG])
@pytest.mark.parametrize("where", ["buffer", "y"])
def test_a_nan_correlation_ranks_first(eng, S, where):
    """One NaN in the buffer makes every correlation of that stream NaN, one in y a run of lags: torch.argmax returns the first NaN, and so
    must both layouts at a run-time geometry; the other streams do not notice."""
    geom = README
    cross, search, delay, block = geom
    lags = [200, 17, 111]
    y3, sola3 = planted(geom, 333, lags, seed=56)
    rows = [r % 3 for r in range(S)]
    y, sola = y3[rows].clone(), sola3[rows].clone()
    hit = [1] if S == 3 else [1, 4, S - 1]
    assert all(rows[h] == 1 for h in hit)
    clean = gpu_tail(eng, y, sola, geom)
    assert clean[2].tolist() == [lags[c] for c in rows]
    for h in hit:
        if where == "buffer":
            sola[h, 123] = float("nan")
        else:
            temp_wav(y, geom)[h, 300] = float("nan")       # lags 61 .. 240 cover it
    with oracle_one_thread():
        _o, _b, ref_shift, ref_corr = oracle(y[hit[:1]], sola[hit[:1]], geom)
    want = ref_shift[0]
    assert want == (0 if where == "buffer" else 300 - cross + 1) and bool(torch.isnan(ref_corr[0][want]))
    out, buf, shift = gpu_tail(eng, y, sola, geom)
    assert int(shift.min()) >= 0 and int(shift.max()) <= search
    assert [int(shift[h]) for h in hit] == [want] * len(hit)
    keep = torch.ones(S, dtype=torch.bool)
    keep[hit] = False
    assert torch.equal(shift[keep], clean[2][keep])
    assert same_bits(out[keep], clean[0][keep]) and same_bits(buf[keep], clean[1][keep])


# ----------------------------------------------------------------------------------------------- nothing is written next to the outputs
@pytest.mark.parametrize("geom,S", [(g, 3) for g in GEOMS] + [(MINIMAL, S_ONE_WG), (ONE_PER_GROUP, S_ONE_WG)], ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("pv", [False, True])
def test_the_neighbours_of_out_buffer_and_shift_stay_untouched(eng, geom, S, pv):
    """tvc_sola_geom_f32 on pointers into the middle of poisoned allocations: out [S][block], sola_buf [S][cross] and shift [S] are written,
    the 64 elements before and after each are not, and what is written is what Engine.sola gives."""
    cross, search, delay, block = geom
    PAD = 64
    lags = random_lags(geom, 3, 77)
    y3, sola3 = planted(geom, 5, lags, seed=6000 + cross)
    rows = [r % 3 for r in range(S)]
    y, sola = y3[rows].contiguous().to(DEV), sola3[rows].contiguous()
    want_out, want_buf, want_shift = gpu_tail(eng, y.cpu(), sola, geom, pv)
    out = torch.full((S * block + 2 * PAD,), 777.0, device=DEV)
    buf = torch.full((S * cross + 2 * PAD,), 777.0, device=DEV)
    buf[PAD:PAD + S * cross] = sola.to(DEV).flatten()
    shift = torch.full((S + 2 * PAD,), -777, dtype=torch.int32, device=DEV)
    fi = fade(cross).to(DEV)
    ptr = lambda t, off: ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    rc = eng.lib.tvc_sola_geom_f32(eng.ctx, eng._stream(), ptr(y, 0), ptr(buf, PAD), ptr(fi, 0), ptr(out, PAD), ptr(shift, PAD), S, y.shape[1], block,
                                   cross, search, delay, int(pv))
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.tvc_last_error(eng.ctx)
    for t, n, poison in ((out, S * block, 777.0), (buf, S * cross, 777.0), (shift, S, -777)):
        assert bool((t[:PAD] == poison).all()) and bool((t[PAD + n:] == poison).all()), "written outside its rows"
    assert torch.equal(shift[PAD:PAD + S].cpu().long(), want_shift)
    assert same_bits(out[PAD:PAD + S * block].cpu().view(S, block), want_out) and same_bits(buf[PAD:PAD + S * cross].cpu().view(S, cross), want_buf)


# ----------------------------------------------------------------------------------------------- phase vocoder
# Inputs: the first seeds from PV_FIRST_SEED upward that meet the preconditions, found on the CPU when the test runs; the planted lags cycle
# through PV_LAGS.  The bound holds per input, as in tests/test_gpu_sola.py - also at cross = 4, where a head is four samples, three of which
# can be off at all: the run-time vocoder evaluates the formula in fp64 and rounds once, so each sample is the fp32 value nearest the truth
# and no fp32 evaluation can be nearer.  (An fp32 run-time vocoder, measured on an MI355X before: per-input ratios of 0.6 .. 2.8 at cross = 4.)
PV_FIRST_SEED = {MINIMAL: 1, README: 15, NEAR_CAPS: 22}
PV_LAGS = {MINIMAL: [0], README: [0, 31, 117, 240, 30, 62, 216, 239], NEAR_CAPS: [0, 240, 1203, 1919]}
PV_INPUTS = {MINIMAL: 48, README: 8, NEAR_CAPS: 4}


def pv_input(geom, seed, lag):
    """(y [Ly], buffer [cross]) of a vocoder input, as tests/test_gpu_sola.py's pv_input: buffer and head are five harmonics of two pitches
    at arbitrary phases (0.03 each) over white noise (0.08; half of the head's noise is the buffer's, which makes the planted lag
    decisive); the head sits at `lag` of an otherwise quiet y."""
    cross, search, delay, block = geom
    g = np.random.default_rng(seed)
    t = np.arange(cross)

    def harm(f0):
        return sum(0.03 * np.sin(2 * np.pi * f0 * (h + 1) * t / 48000.0 + g.uniform(0, 2 * np.pi)) for h in range(5))

    na, nb = g.standard_normal(cross), g.standard_normal(cross)
    a = harm(g.uniform(100, 400)) + 0.08 * na
    b = harm(g.uniform(100, 400)) + 0.08 * (0.5 * na + math.sqrt(0.75) * nb)
    y = torch.from_numpy((0.01 * g.standard_normal(min_ly(geom) + 7)).astype(np.float32))
    temp_wav(y, geom)[lag:lag + cross] = torch.from_numpy(b.astype(np.float32))
    return y, torch.from_numpy(a.astype(np.float32))


def pv_preconditions(a, b, cross):
    """tests/test_gpu_sola.py's, at `cross`: (smallest bin magnitude / largest, smallest distance of dp / 2 pi + 0.5 from an integer over
    the bins strictly between 0 and Nyquist) on the fp64 spectra of the windowed buffer and head"""
    fi = fade(cross).double()
    w = torch.sqrt((1 - fi) * fi)
    fa, fb = torch.fft.rfft(a.double() * w), torch.fft.rfft(b.double() * w)
    mags = torch.cat([fa.abs(), fb.abs()])
    x = ((torch.angle(fb) - torch.angle(fa)) / 2 / math.pi + 0.5)[1:-1]
    return float(mags.min() / mags.max()), float((x - torch.round(x)).abs().min())


def pv_inputs(geom):
    """-> (y [n, Ly], buffers [n, cross], lags, seeds): PV_INPUTS inputs that meet the preconditions - the planted lag
    is the fp64 arg-max by more than fp32 can move it, no bin is below 1e-3 of the largest, no inner bin within 1e-3 of the phase wrap"""
    cross, search, delay, block = geom
    n = PV_INPUTS[geom]
    ys, solas, lags, seeds = [], [], [], []
    seed = PV_FIRST_SEED[geom]
    while len(ys) < n:
        assert seed < PV_FIRST_SEED[geom] + 8 * n + 64, f"precondition: only {len(ys)} of {n} usable inputs"
        lag = PV_LAGS[geom][len(ys) % len(PV_LAGS[geom])]
        y, sola = pv_input(geom, seed, lag)
        floor, wrap = pv_preconditions(sola, temp_wav(y, geom)[lag:lag + cross], cross)
        if floor >= 1e-3 and wrap >= 1e-3:
            corr64 = oracle(y[None], sola[None], geom, dtype=torch.float64)[3][0]
            best, g = gap(corr64)
            if best == lag and g > decidable_bound(sola, cross):
                ys.append(y), solas.append(sola), lags.append(lag), seeds.append(seed)
        seed += 1
    return torch.stack(ys), torch.stack(solas), lags, seeds


@pytest.mark.parametrize("geom", list(PV_INPUTS), ids=gid)
def test_phase_vocoder_against_fp64(eng, geom):
    """The vocoder head at cross = 4, 240 and 1916 against the fp64 evaluation of the reference's formula, under the bound
    tests/test_gpu_sola.py applies at 1920: per input, the kernel may be at most twice as far from the truth as the reference's own fp32
    evaluation (one thread).  Everything outside the head is a copy and is compared to the bit."""
    cross, search, delay, block = geom
    y, sola, lags, seeds = pv_inputs(geom)
    n = len(lags)
    out64, buf64, shift64, _c = oracle(y, sola, geom, pv=True, dtype=torch.float64)
    with oracle_one_thread():
        out32, buf32, shift32, _c = oracle(y, sola, geom, pv=True)
    assert shift64 == lags and shift32 == lags
    out, buf, shift = gpu_tail(eng, y, sola, geom, pv=True)
    assert shift.tolist() == lags
    assert torch.isfinite(out).all() and torch.isfinite(buf).all()
    # the head: the first cross samples of [out | next buffer]
    heads = lambda o, b: torch.stack([torch.cat([torch.as_tensor(o[i]), torch.as_tensor(b[i])])[:cross].double() for i in range(n)])
    truth, h_gpu, h_ref = heads(out64, buf64), heads(out, buf), heads(out32, buf32)
    figures = [(rms(h_gpu[i] - truth[i]), rms(h_ref[i] - truth[i])) for i in range(n)]
    ratios = [g / r for g, r in figures if r > 0]
    _log(f"[parity] vocoder head {gid(geom)}: {n} inputs (seeds {seeds[0]} .. {seeds[-1]}), rms err gpu {rms(h_gpu - truth):.3e} oracle-fp32 {rms(h_ref - truth):.3e} over all; "
         f"per input gpu / oracle-fp32: worst {max(ratios):.3f}, best {min(ratios):.3f}; signal rms {rms(truth):.3e}")
    for i, (e_gpu, e_ref) in enumerate(figures):
        assert e_gpu <= 2 * e_ref, f"{gid(geom)} input {i} (seed {seeds[i]}): head rms error {e_gpu:.3e} > 2 x {e_ref:.3e} (the fp32 oracle's)"
    for i in range(n):
        both = torch.cat([out[i], buf[i]])
        tw = temp_wav(y[i], geom)
        assert same_bits(both[cross:], tw[lags[i] + cross:lags[i] + cross + block]), f"input {i}: behind the head everything is a copy"


# ----------------------------------------------------------------------------------------------- the two entries, refusals
@pytest.mark.parametrize("pv", [False, True])
def test_the_default_geometry_is_tvc_sola_f32_bit_for_bit(eng, pv):
    """Engine.sola with no geometry keyword calls tvc_sola_f32 (which keeps its own error text, tests/test_gpu_sola.py), with any of them
    tvc_sola_geom_f32: this test runs both entries on the same rows."""
    from test_gpu_sola import voiced_case
    block = 960
    y, sola = voiced_case(5, block, 333, seed=2025)
    dy, fi = y.to(DEV), fade(1920).to(DEV)
    a_buf, b_buf = sola.to(DEV).clone(), sola.to(DEV).clone()
    a_out, a_shift = eng.sola(dy, a_buf, fi, block, use_phase_vocoder=pv, want_shift=True)
    b_out, b_shift = eng.sola(dy, b_buf, fi, block, use_phase_vocoder=pv, want_shift=True, crossfade=1920, search=1920, delay=3840)
    torch.cuda.synchronize()
    assert len(set(a_shift.tolist())) > 1 and torch.equal(a_shift, b_shift)
    assert same_bits(a_out.cpu(), b_out.cpu()) and same_bits(a_buf.cpu(), b_buf.cpu()) and not same_bits(a_buf.cpu(), sola)
    # a keyword left out is the reference's value
    c_buf = sola.to(DEV).clone()
    c_out = eng.sola(dy, c_buf, fi, block, use_phase_vocoder=pv, delay=3840)
    assert same_bits(a_out.cpu(), c_out.cpu()) and same_bits(a_buf.cpu(), c_buf.cpu())


def test_refusals_carry_the_librarys_message(eng):
    from tinyvc_amd._lib import TinyVCError
    keep = torch.full((2, 240), 0.25)
    buf = keep.to(DEV)
    y = torch.zeros(2, 1440, device=DEV)

    def call(y=y, buf=buf, block=480, cross=240, search=240, delay=480, n_fade=None):
        return eng.sola(y, buf, fade(240 if n_fade is None else n_fade).to(DEV), block, crossfade=cross, search=search, delay=delay)
    for kw, text in ((dict(search=-1), "search = -1 is outside 0 .. 1920"), (dict(search=1921), "search = 1921"), (dict(delay=-1), "delay = -1 is negative"),
                     (dict(block=0), "block = 0 is not positive"), (dict(y=y[:, :1439]), "Ly = 1439 is shorter than block \\+ cross \\+ search \\+ delay = 1440"),
                     (dict(delay=481), "= 1441")):
        with pytest.raises(TinyVCError, match="tvc_sola_geom_f32: .*" + text):
            call(**kw)
    # the cross-fade length is the two tensors' length: a mismatch never reaches the kernels, an illegal one is the library's refusal
    for kw in (dict(cross=480), dict(n_fade=244), dict(buf=torch.zeros(2, 244, device=DEV))):
        with pytest.raises(ValueError, match="crossfade = "):
            call(**kw)
    for cross, text in ((6, "cross = 6 is not a multiple of 4"), (1924, "cross = 1924 is outside 4 .. 1920"), (2, "cross = 2")):
        with pytest.raises(TinyVCError, match="tvc_sola_geom_f32: " + text):
            eng.sola(torch.zeros(2, 9600, device=DEV), torch.zeros(2, cross, device=DEV), torch.zeros(cross, device=DEV), 480, crossfade=cross, search=240, delay=480)
    for kw in (dict(cross=240.9), dict(search=240.0), dict(delay="480"), dict(delay=True)):
        with pytest.raises(ValueError, match="must be an integer"):
            call(**kw)
    torch.cuda.synchronize()
    assert same_bits(buf.cpu(), keep), "a refused call must not touch the buffer"
    assert call().shape == (2, 480)      # the shortest accepted row


# ----------------------------------------------------------------------------------------------- streams
S = 3
KW = dict(crossfade_size=240, sola_search_size=240, last_delay_size=480, block_size=480)
N_BLOCKS = 8


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


@pytest.fixture(scope="module")
def model_side():
    tgt = synth.synth_index(500, seed=2).to(DEV)
    blocks = synth.synth_wave(S, N_BLOCKS * 480, seed=50).view(S, N_BLOCKS, 480).to(DEV)
    angles = [synth.synth_angle(S, 9, 700 + i).to(DEV) for i in range(N_BLOCKS)]      # 4320-sample windows: 9 frames
    return tgt, blocks, angles


def _stream(gen, tgt, use_graph=False, **kw):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    args = dict(n_streams=S, target=tgt, pitch_shift=[0.0, 2.0, -1.5], device=torch.device(DEV), extra_size=3840, use_graph=use_graph)
    args.update(KW)
    args.update(kw)
    st = BatchedStreamInfer(gen, **args)
    st.init_buffer()
    return st


def _class_loop(gen, model_side, use_graph):
    tgt, blocks, angles = model_side
    st = _stream(gen, tgt, use_graph)
    outs, shifts, graphs = [], [], []
    for i in range(N_BLOCKS):
        outs.append(st.audio_callback(blocks[:, i], noise_angle=angles[i]).clone())
        shifts.append(st.last_shift.clone())
        graphs.append(st._graph[1][True][0] if use_graph and st._graph is not None and True in st._graph[1] else None)
    return torch.stack(outs), torch.stack(shifts), graphs, st


@pytest.fixture(scope="module")
def eager(gen, model_side):
    return _class_loop(gen, model_side, False)


def test_a_stream_at_the_short_geometry_equals_the_hand_written_loop(gen, model_side, eager):
    tgt, blocks, angles = model_side
    st = eager[3]
    assert st.input_size == 4320 and st.sola_buffer.shape == (S, 240) and st.fade_in_window.shape == (240,)
    assert st.latency_samples == (720, 960) and st.latency_seconds == (0.03, 0.04)
    dev = torch.device(DEV)
    eng = gen.engine(dev)
    wav = torch.zeros(S, 4320, device=dev)
    buf = torch.zeros(S, 240, device=dev)
    fi = fade(240).to(dev)
    for i in range(N_BLOCKS):
        eng.stream_push(wav, blocks[:, i].contiguous())
        y = gen.convert(wav, tgt, [0.0, 2.0, -1.5], device=dev, noise_angle=angles[i])
        out, shift = eng.sola(y, buf, fi, 480, want_shift=True, crossfade=240, search=240, delay=480)
        assert torch.equal(shift, eager[1][i]) and int(shift.max()) <= 240, f"block {i}"
        assert torch.equal(out, eager[0][i]), f"block {i}"
    assert len(set(eager[1].flatten().tolist())) > 3, "the stream must have searched"
    assert torch.equal(buf, st.sola_buffer) and float(eager[0][2:].abs().max()) > 1e-3


def test_graph_replay_equals_eager_with_one_capture(gen, model_side, eager):
    graph = _class_loop(gen, model_side, True)
    g = graph[2]
    assert g[0] is None and g[1] is None and g[2] is not None and all(x is g[2] for x in g[2:]), "a block captured a new graph"
    assert torch.equal(eager[1], graph[1]), "SOLA lags differ between eager and graph replay"
    assert torch.equal(eager[0], graph[0]), "graph replay is not sample-exact"
    # the geometry is part of the key; an attribute changed after construction is refused until init_buffer() follows it, then honoured
    st = graph[3]
    key = st._graph_key()
    assert key == st._graph[0]
    keep = st.sola_buffer.clone()
    for name, value in (("sola_search_size", 100), ("last_dilay_size", 960), ("crossfade_size", 480)):
        old = getattr(st, name)
        setattr(st, name, value)
        assert st._graph_key() != key
        with pytest.raises(ValueError, match="call init_buffer"):
            st.audio_callback(model_side[1][:, 0], noise_angle=model_side[2][0])
        setattr(st, name, old)
        assert st._graph_key() == key
    assert torch.equal(st.sola_buffer, keep), "a refused block touched the buffer"
    st.crossfade_size, st.last_dilay_size = 480, 960
    st.init_buffer()
    assert st.input_size == max(480 + 480 + 240 + 2 * 960, 480 + 3840), "init_buffer follows the attributes"
    assert st.sola_buffer.shape == (S, 480) and st.audio_callback(model_side[1][:, 0], noise_angle=model_side[2][0]).shape == (S, 480)


def _oracle_stream(blocks, tgt, nthreads, extra):
    """oracle.ref_cpu.stream_callback over the blocks of one stream, on a StreamState set to KW's geometry -> [(out, lag)]"""
    enc_sd, dec_sd = state_dicts(0)
    ost = R.StreamState(block_size=480, extra_size=extra)
    ost.cross, ost.search, ost.delay = 240, 240, 480
    ost.input_size = max(ost.block + ost.cross + ost.search + 2 * ost.delay, ost.block + extra)
    frames = -(-ost.input_size // 480)
    ost.fade_in = fade(240)
    ost.fade_out = 1 - ost.fade_in
    ost.input_wav = torch.zeros(ost.input_size)
    ost.sola = torch.zeros(ost.cross)
    keep = torch.get_num_threads()
    torch.set_num_threads(nthreads)
    try:
        return [R.stream_callback(ost, enc_sd, dec_sd, tgt, 1.0, blocks[i], synth.synth_angle(1, frames, 4000 + i)) for i in range(N_BLOCKS)]
    finally:
        torch.set_num_threads(keep)


@pytest.mark.parametrize("extra", [3840, 3940], ids=["whole-frames", "padded-window"])
def test_a_stream_at_the_short_geometry_against_the_oracle_loop(gen, extra):
    """One stream over 8 blocks against oracle.ref_cpu.stream_callback (= reference stream.py:68-96) at the same geometry, fed the same
    blocks and noise phases: lags identical, every block within 1e-4 rms.  A lag is an arg-max over near-tied values of a quasi-periodic
    signal; as in tests/test_gpu_cfg3.py's chunked test the input is the first seed on which the oracle agrees with itself on every lag
    between 1 and several threads.
    extra_size = 3940: a 4420-sample window, which both sides convert as 4800 (zeros behind the end) and cut the tail from the END of: the
    look-ahead over the signal is 480 - 380 samples, which latency_samples says, and the block is still the oracle's.""" 
    from tinyvc_amd.module.infer import StreamInfer
    tgt = synth.synth_index(300, seed=2)
    nthr = min(8, torch.get_num_threads())
    for seed in range(82, 92):
        blocks = synth.synth_wave(1, N_BLOCKS * 480, seed=seed)[0].view(N_BLOCKS, 480)
        ref, ref1 = _oracle_stream(blocks, tgt, nthr, extra), _oracle_stream(blocks, tgt, 1, extra)
        if all(a[1] == b[1] for a, b in zip(ref, ref1)):
            break
        print(f"[geometry] seed {seed}: the oracle's own lags differ between 1 and {nthr} threads (near-tied arg-max): next seed")
    else:
        pytest.fail("no decidable input found")
    assert ref1[0][1] == 0 and len({r[1] for r in ref1}) > 2, "the oracle stream must have searched"
    st = StreamInfer(gen, target=tgt.to(DEV), pitch_shift=1.0, device=torch.device(DEV), extra_size=extra, **KW)
    frames = -(-st.input_size // 480)
    assert (st.input_size, st.pad_size, st.latency_samples) == ((4320, 0, (720, 960)) if extra == 3840 else (4420, 380, (340, 580)))
    st.init_buffer()
    worst = 0.0
    for i in range(N_BLOCKS):
        out = st.audio_callback(blocks[i].to(DEV), noise_angle=synth.synth_angle(1, frames, 4000 + i).to(DEV)).cpu()
        lag = int(st.last_shift[0])
        d = rms(out - ref1[i][0])
        worst = max(worst, d)
        _log(f"[parity] stream 240/240/480 block 480 window {st.input_size} (seed {seed}) block {i}: lag {lag} (oracle {ref1[i][1]}), rms diff {d:.3e}")
        assert lag == ref1[i][1], f"block {i}: SOLA lag {lag} != oracle {ref1[i][1]}"
        assert d <= 1e-4, f"block {i}: rms diff {d:.3e}"
    assert worst > 0.0


def test_auto_pitch_takes_a_whole_frame_look_ahead(gen, model_side):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    tgt, blocks, angles = model_side
    with pytest.raises(ValueError, match="last_delay_size = 500 is not a whole number of 480-sample frames"):
        BatchedStreamInfer(gen, n_streams=S, target=tgt, device=torch.device(DEV), extra_size=3840, auto_pitch=200.0, crossfade_size=240, sola_search_size=240,
                           last_delay_size=500, block_size=480)
    st = _stream(gen, tgt, auto_pitch=200.0, last_delay_size=960, pitch_shift=0.0)
    assert (st.pitch_track.new_frames, st.pitch_track.lag_frames) == (1, 2), "the tracker's new frames end last_dilay_size // 480 = 2 frames before the end"
    for i in range(4):
        out = st.audio_callback(blocks[:, i], noise_angle=angles[i])
    assert out.shape == (S, 480) and bool(torch.isfinite(out).all()) and st.last_pitch_shift.shape == (S,) and int(st.last_shift.max()) <= 240


def test_windows_the_front_end_or_the_tail_cannot_take_are_refused_in_the_constructor(gen):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    short = dict(n_streams=S, device=torch.device(DEV), block_size=480, crossfade_size=100, sola_search_size=100, last_delay_size=100)
    with pytest.raises(ValueError, match="window of 880 samples"):
        BatchedStreamInfer(gen, **short)
    with pytest.raises(ValueError, match="window of 961 samples is converted as 1440"):      # 479 samples of padding behind a look-ahead of 100
        BatchedStreamInfer(gen, extra_size=481, **short)
    st = BatchedStreamInfer(gen, target=synth.synth_index(300, seed=2).to(DEV), extra_size=960, **short)
    st.init_buffer()      # 1440 samples, whole frames: runs
    out = st.audio_callback(torch.zeros(S, 480, device=DEV), noise_angle=synth.synth_angle(S, 3, 1).to(DEV))
    assert st.input_size == 1440 and out.shape == (S, 480) and bool(torch.isfinite(out).all())
    # a padded window as a captured graph that draws its own phases: one column per frame of the padded window
    st = BatchedStreamInfer(gen, n_streams=S, target=synth.synth_index(300, seed=2).to(DEV), device=torch.device(DEV), extra_size=3940, use_graph=True, **KW)
    st.init_buffer()
    for _ in range(4):
        out = st.audio_callback(torch.zeros(S, 480, device=DEV))
    assert st.pad_size == 380 and st._graph is not None and out.shape == (S, 480) and bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------------------------- the entry script
def test_infer_streaming_with_the_three_flags_equals_the_class_loop(tmp_path, capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor
    d = tmp_path
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(500, seed=2), d / "index.pt")
    audio_io.save(str(d / "mic.wav"), synth.synth_wave(3, 12 * 480, seed=50)[0:1] * 0.9, 24000)
    torch.manual_seed(3)
    assert infer_streaming.main(["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "index.pt"), "--input-wav", str(d / "mic.wav"),
                                 "--streams", "2", "-d", DEV, "-p", "0.5", "-c", "480", "--crossfade", "240", "--sola-search", "240", "--lookahead", "480",
                                 "--output-wav", str(d / "short.wav")]) == 0
    text = capsys.readouterr().out
    assert "Latency 30.0 to 40.0 ms" in text and "plus the 20 ms block" in text
    torch.manual_seed(3)
    dev = torch.device(DEV)
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), dev)
    door = StreamDoor(2, 24000, block_size=480, device=dev)
    st = BatchedStreamInfer(gen, n_streams=2, pitch_shift=0.5, device=dev, extra_size=3840, door=door, **KW)
    st.target = torch.load(d / "index.pt").to(dev)
    st.init_buffer()
    outs = []
    for blk in infer_streaming.int16_blocks_from_wav(str(d / "mic.wav"), 24000, 480, gen.engine(dev)):
        pcm = torch.from_numpy(np.ascontiguousarray(blk)).to(dev)
        outs.append(st.audio_callback_pcm(pcm.expand(2, -1)).cpu().numpy()[0])
    assert len(outs) == 12 and int(np.abs(np.concatenate(outs).astype(np.int32)).max()) > 100
    audio_io.save(str(d / "want.wav"), torch.from_numpy(np.concatenate(outs).astype(np.float32) / 32768)[None], 24000)
    assert open(d / "short.wav", "rb").read() == open(d / "want.wav", "rb").read()
