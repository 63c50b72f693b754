"""The streaming tail (tvc_sola_f32: lag search, sin^2 cross-fade, phase vocoder, in-place buffer update; and the rolling
buffer push) kernel by kernel, on synthetic seeded inputs, through Engine.sola / Engine.stream_push of a weightless engine.

Truth is oracle.ref_cpu.sola_tail on float64 copies of the inputs; the float32 call of the same function is what the
reference computes and is the bit-for-bit reference of everything that is not a sum (the cross-fade is three fp32 roundings,
the rest are copies).  A lag is compared only where float32 can decide it: the fp64 gap between the best and the second-best
correlation is asserted, never skipped, with seeds that were chosen on the CPU so that it holds.

Two launch layouts are run wherever a lag is checked: S <= 1024 streams take the split search (sola_corr_kernel, 8 lag groups
of 241 per stream), S = 1025 the one-workgroup search inside sola_kernel (lags strided by 256 over the threads).
The whole file takes about 9 s."""
import math

import numpy as np
import pytest
import torch

from helpers import oracle_one_thread, rms
from oracle import ref_cpu as R
from test_gpu_parity import _log          # the [parity] lines of this file go where the other parity figures go

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CROSS = SEARCH = 1920
DELAY = 3840
S_ONE_WG = 1025                     # the first S past the split search's scratch (tvc_common.h: kSolaPartFloats / 16 = 1024)
FADE = torch.sin(math.pi * torch.arange(0, 1, 1 / CROSS) / 2) ** 2          # StreamState.fade_in
# group seams of the split search (240/241, 481/482, 1445/1446, 1686/1687), its shortened last group (1920), wave seams (63/64)
# and the 255/256 stride of the one-workgroup loop
LAGS = [0, 1, 63, 64, 239, 240, 241, 242, 255, 256, 481, 482, 1445, 1446, 1686, 1687, 1688, 1919, 1920]
MIN_LY = CROSS + SEARCH + DELAY         # Ly >= block + 7680
LY_EXTRA = [0, 333, 1920]           # Ly above the minimum; 333: rows that do not start on a multiple of 4 floats


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


# ----------------------------------------------------------------------------------------------- the only device access
def gpu_tail(eng, y, sola, block, pv=False):
    """Engine.sola on host tensors y [S, Ly], sola [S, 1920] -> (out [S, block], new buffer [S, 1920], shift [S]) on the host."""
    buf = sola.to(DEV).clone()
    out, shift = eng.sola(y.to(DEV), buf, FADE.to(DEV), block, use_phase_vocoder=pv, want_shift=True)
    torch.cuda.synchronize()
    return out.cpu(), buf.cpu(), shift.cpu().long()


def gpu_push(eng, buf, blocks):
    d = buf.to(DEV).clone()
    eng.stream_push(d, blocks.to(DEV))
    torch.cuda.synchronize()
    return d.cpu()


# ----------------------------------------------------------------------------------------------- references
def temp_wav(y, block):
    """The window of y the tail works on (stream.py:74), [.., block + 3840]."""
    return y[..., y.shape[-1] - block - CROSS - SEARCH - DELAY:y.shape[-1] - DELAY]


def np_tail(y, sola, shift, block):
    """The sin^2 tail at a given lag in plain numpy float32: products and the sum rounded one by one, everything else a copy."""
    tw = temp_wav(y, block).numpy()
    fi = FADE.numpy()
    seg = tw[shift:shift + block + CROSS]
    head = seg[:CROSS] * fi + sola.numpy() * (np.float32(1) - fi)
    assert head.dtype == np.float32
    temp = np.concatenate([head, seg[CROSS:]])
    return temp[:block], temp[block:], head


def oracle(y, sola, block, pv=False, dtype=torch.float32):
    """R.sola_tail per stream -> lists of out, new buffer, shift, corr."""
    res = [R.sola_tail(y[s].to(dtype), sola[s].to(dtype), FADE.to(dtype), block, pv) for s in range(y.shape[0])]
    return [list(c) for c in zip(*res)]


def gap64(corr):
    """(best lag, gap between the best and the second-best value) of an fp64 correlation."""
    top = torch.topk(corr, 2)
    return int(torch.argmax(corr)), float(top.values[0] - top.values[1])


def decidable_bound(sola):
    """What a 1920-term fp32 sum can move a correlation by: |nom| / ||window|| <= ||sola||, each of the two compared values within
    1920 * 2^-24 of its own."""
    return 2 * CROSS * 2.0 ** -24 * float(sola.double().norm())


def same_bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def first_diff(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    bad = (a.view(torch.int32) != b.view(torch.int32)).flatten().nonzero()
    i = int(bad[0]) if len(bad) else -1
    return f"{len(bad)} of {a.numel()} differ, first at {i}: {float(a.flatten()[i])!r} vs {float(b.flatten()[i])!r}"


def layouts(n):
    """Row maps of the two launch layouts: every case once (split search), and S_ONE_WG streams cycling through the cases."""
    return [("split", list(range(n))), ("one-wg", [r % n for r in range(S_ONE_WG)])]


def voiced(rows, n, seed, noise=1e-3):
    """[rows, n] quasi-periodic rows at 0.1 rms: 8 harmonics of a glide between two pitches in 70 .. 500 Hz (at 48 kHz) with a slow
    vibrato, like tests/test_gpu_long.py's f0 runs, plus a little white noise.  Neighbouring pitch periods correlate almost equally
    well: the near ties a lag search meets in speech."""
    g = np.random.default_rng(seed)
    t = np.arange(n)
    out = np.empty((rows, n), np.float32)
    for r in range(rows):
        a, z = g.uniform(70.0, 500.0, 2)
        f = np.geomspace(a, z, n) * (1 + 0.01 * np.sin(t * g.uniform(2e-4, 2e-3)))
        ph = 2 * np.pi * np.cumsum(f) / 48000.0
        amp = g.uniform(0.2, 1.0, 8) / np.arange(1, 9)
        x = sum(amp[h] * np.sin((h + 1) * ph + g.uniform(0, 2 * np.pi)) for h in range(8))
        out[r] = 0.1 * x / np.sqrt(np.mean(x * x)) + noise * g.standard_normal(n)
    return torch.from_numpy(out)


def voiced_case(rows, block, extra, seed):
    """(y [rows, Ly], buffer [rows, 1920]): the buffer is what a previous block would have left, a window of the same signal somewhere
    in the search range, scaled and with its own noise."""
    Ly = block + MIN_LY + extra
    y = voiced(rows, Ly, seed)
    g = np.random.default_rng(seed + 1)
    tw = temp_wav(y, block)
    sola = torch.empty(rows, CROSS)
    for r in range(rows):
        lag = int(g.integers(0, SEARCH + 1))
        sola[r] = 0.8 * tw[r, lag:lag + CROSS] + torch.from_numpy(0.005 * g.standard_normal(CROSS).astype(np.float32))
    return y, sola


# ----------------------------------------------------------------------------------------------- planted lags
def planted(block, extra, seed):
    n = len(LAGS)
    g = torch.Generator().manual_seed(seed)
    Ly = block + MIN_LY + extra
    y = 0.1 * torch.randn(n, Ly, generator=g)
    sola = 0.1 * torch.randn(n, CROSS, generator=g)
    tw = temp_wav(y, block)
    for s, lag in enumerate(LAGS):
        tw[s, lag:lag + CROSS] = 0.7 * sola[s]
    return y, sola


@pytest.mark.parametrize("extra", LY_EXTRA)
@pytest.mark.parametrize("block", [480, 960, 1920, 9600])
def test_planted_lags_and_the_sin2_tail_to_the_bit(eng, block, extra):
    """A copy of the buffer planted at every seam of the work split: the lag is found, and the block and the next buffer are the fp32
    oracle's, and plain numpy's, to the bit - on both search branches, for every stream of the call."""
    y, sola = planted(block, extra, seed=1000 + block + extra)
    n = len(LAGS)
    _o, _b, _s, corr64 = oracle(y, sola, block, dtype=torch.float64)
    for s, lag in enumerate(LAGS):
        best, gap = gap64(corr64[s])
        assert best == lag and gap >= 0.5, f"precondition: planted lag {lag} is not decisive in fp64 (best {best}, gap {gap:.3f})"
    with oracle_one_thread():
        ref_out, ref_buf, ref_shift, _c = oracle(y, sola, block)
    assert ref_shift == LAGS
    for name, rows in layouts(n):
        # (one-wg: each cycle through the cases is scaled by another power of two, which scales every product and sum of the tail
        # exactly - no value comes near the subnormals - so the rows differ and the oracle's rows still apply)
        scale = torch.tensor([2.0 ** -(r // n % 4) for r in range(len(rows))])[:, None]
        yy, ss = y[rows] * scale, sola[rows] * scale
        out, buf, shift = gpu_tail(eng, yy, ss, block)
        assert shift.tolist() == [LAGS[c] for c in rows], f"{name}: lags {shift.tolist()[:2 * n]} ..."
        for r, c in enumerate(rows):
            what = f"{name} block {block} Ly +{extra} stream {r} (lag {LAGS[c]})"
            e_out, e_buf, head = np_tail(yy[r], ss[r], LAGS[c], block)
            assert same_bits(out[r], e_out), f"{what}: out vs numpy: {first_diff(out[r], e_out)}"
            assert same_bits(buf[r], e_buf), f"{what}: buffer vs numpy: {first_diff(buf[r], e_buf)}"
            assert same_bits(out[r], ref_out[c] * scale[r]), f"{what}: out vs oracle: {first_diff(out[r], ref_out[c] * scale[r])}"
            assert same_bits(buf[r], ref_buf[c] * scale[r]), f"{what}: buffer vs oracle: {first_diff(buf[r], ref_buf[c] * scale[r])}"
            if block < CROSS:
                # the next buffer: the rest of the cross-faded head, then raw samples behind it
                tw = temp_wav(yy[r], block)
                assert same_bits(buf[r, :CROSS - block], head[block:]), f"{what}: buffer[:{CROSS - block}] is not the faded head's rest"
                assert same_bits(buf[r, CROSS - block:], tw[LAGS[c] + CROSS:LAGS[c] + CROSS + block]), \
                    f"{what}: buffer[{CROSS - block}:] is not the samples behind the head"
                assert same_bits(out[r], head[:block])


# ----------------------------------------------------------------------------------------------- carried state + rolling buffer
@pytest.mark.parametrize("block,seed", [(960, 37), (1920, 32)])
def test_six_blocks_of_carried_state(eng, block, seed):
    """Six consecutive blocks on 3 streams, the rolling input pushed by Engine.stream_push and the buffer fed back: lag, block and
    buffer equal the oracle loop's at every step.  The first block starts from the all-zero buffer: every lag ties at 0.  A converter
    does not place its output at the same sample from call to call, which is what the search is for: each call reads the rolling
    signal at its own offset (per stream, 0 .. 1920), so the lags move."""
    S, Ly = 3, block + MIN_LY + 333
    Lr = Ly + SEARCH
    sig = voiced(S, Lr + 6 * block, seed, noise=3e-3)
    jitter = np.random.default_rng(seed).integers(0, SEARCH + 1, (6, S))
    roll_g, roll_r = sig[:, :Lr].clone(), sig[:, :Lr].clone()
    sola_g, sola_r, sola_64 = torch.zeros(S, CROSS), torch.zeros(S, CROSS), torch.zeros(S, CROSS, dtype=torch.float64)
    lags = []
    for k in range(6):
        new = sig[:, Lr + k * block:Lr + (k + 1) * block]
        roll_r = torch.roll(roll_r, -block, 1)
        roll_r[:, -block:] = new
        roll_g = gpu_push(eng, roll_g, new)
        assert same_bits(roll_g, roll_r), f"block {k}: stream_push: {first_diff(roll_g, roll_r)}"
        y = torch.stack([roll_g[s, j:j + Ly] for s, j in enumerate(jitter[k])])
        _o, buf64, shift64, corr64 = oracle(y, sola_64, block, dtype=torch.float64)
        with oracle_one_thread():
            ref_out, ref_buf, ref_shift, _c = oracle(y, sola_r, block)
        for s in range(S):
            best, gap = gap64(corr64[s])
            if k == 0:
                assert best == 0 and gap == 0.0 and float(corr64[s].abs().max()) == 0.0
            else:
                assert gap > decidable_bound(sola_r[s]) and best == ref_shift[s], \
                    f"precondition: block {k} stream {s} is not decidable in fp32 (gap {gap:.3e}, fp64 lag {best}, fp32 {ref_shift[s]})"
        out, sola_g, shift = gpu_tail(eng, y, sola_g, block)
        _log(f"[parity] sola carried block={block} step {k}: lags {shift.tolist()} (oracle {ref_shift})")
        assert shift.tolist() == ref_shift, f"block {k}"
        for s in range(S):
            assert same_bits(out[s], ref_out[s]), f"block {k} stream {s}: out: {first_diff(out[s], ref_out[s])}"
            assert same_bits(sola_g[s], ref_buf[s]), f"block {k} stream {s}: buffer: {first_diff(sola_g[s], ref_buf[s])}"
        sola_r, sola_64 = torch.stack(ref_buf), torch.stack(buf64)
        lags += ref_shift
    assert len(set(lags)) > 6, f"the later blocks must have searched: {lags}"


# ----------------------------------------------------------------------------------------------- exact ties
TIES = [(100, 37), (100, 99), (241, 0), (241, 240), (241, 17), (256, 5)]


def test_exact_ties_keep_the_lowest_lag(eng):
    """y exactly periodic in fp32, the buffer one window of it: every lag = phase (mod period) sees the same window, hence the same
    sums in the same order, hence the same correlation.  The first maximum is the reference's rule.  Period 241 ties the first (phase 0)
    or the last (phase 240) lag of every group of the split search, period 256 ties the lags of ONE thread of the one-workgroup loop."""
    block = 1920
    Ly = block + MIN_LY + 5
    g = torch.Generator().manual_seed(77)
    y = torch.zeros(len(TIES), Ly)
    sola = torch.zeros(len(TIES), CROSS)
    for c, (P, phi) in enumerate(TIES):
        pat = 0.1 * torch.randn(P, generator=g)
        n = block + CROSS + SEARCH
        temp_wav(y, block)[c] = pat[torch.arange(n) % P]
        sola[c] = pat[(phi + torch.arange(CROSS)) % P]
    _o, _b, shift64, corr64 = oracle(y, sola, block, dtype=torch.float64)
    for c, (P, phi) in enumerate(TIES):
        at_max = (corr64[c] == corr64[c].max()).nonzero().flatten().tolist()
        assert at_max == list(range(phi, SEARCH + 1, P)), f"precondition: period {P} phase {phi}: fp64 maxima at {at_max}"
        assert shift64[c] == phi
    for name, rows in layouts(len(TIES)):
        out, buf, shift = gpu_tail(eng, y[rows], sola[rows], block)
        assert shift.tolist() == [TIES[c][1] for c in rows], f"{name}: {shift.tolist()[:12]} ... for (period, phase) {TIES}"
        for r, c in enumerate(rows):
            e_out, e_buf, _h = np_tail(y[c], sola[c], TIES[c][1], block)
            assert same_bits(out[r], e_out) and same_bits(buf[r], e_buf), f"{name} stream {r}"


@pytest.mark.parametrize("S", [3, S_ONE_WG])
def test_all_zero_input_ties_at_lag_zero(eng, S):
    """All-zero y: every correlation is 0 / sqrt(1e-8) = 0, the lag is 0 and the block is the faded-out buffer; with a zero buffer too,
    everything is zero."""
    block = 960
    y = torch.zeros(S, block + MIN_LY)
    sola = 0.1 * torch.randn(S, CROSS, generator=torch.Generator().manual_seed(5))
    sola[S // 2:] = 0
    out, buf, shift = gpu_tail(eng, y, sola, block)
    assert shift.tolist() == [0] * S
    fade = np.float32(0) * FADE.numpy() + sola.numpy() * (np.float32(1) - FADE.numpy())
    assert same_bits(out, fade[:, :block]) and same_bits(buf[:, :CROSS - block], fade[:, block:])
    assert not buf[:, CROSS - block:].any() and not out[S // 2:].any() and not buf[S // 2:].any()


# ----------------------------------------------------------------------------------------------- branch equivalence
@pytest.mark.parametrize("pv", [False, True])
def test_every_row_of_the_one_workgroup_search_equals_its_own_split_search_call(eng, pv):
    """S = 1025 (one-workgroup search) against the same rows one by one (split search): lag, block and buffer bit for bit, sin^2 and
    vocoder.  No reference is involved, so the near ties of quasi-periodic input are welcome."""
    block = 960
    y, sola = voiced_case(S_ONE_WG, block, 333, seed=2024)
    dy, dsola, fade = y.to(DEV), sola.to(DEV), FADE.to(DEV)
    big = dsola.clone()
    out, shift = eng.sola(dy, big, fade, block, use_phase_vocoder=pv, want_shift=True)
    torch.cuda.synchronize()
    assert int(shift.min()) >= 0 and int(shift.max()) <= SEARCH
    assert len(set(shift.tolist())) > S_ONE_WG // 10, "the rows must exercise many lags"
    o1, b1, s1 = torch.empty_like(out), dsola.clone(), torch.empty_like(shift)
    for r in range(S_ONE_WG):
        o, s = eng.sola(dy[r:r + 1], b1[r:r + 1], fade, block, use_phase_vocoder=pv, want_shift=True)
        o1[r], s1[r] = o[0], s[0]
    torch.cuda.synchronize()
    bad = (shift != s1).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} rows choose another lag alone, first row {bad[0]}: {int(shift[bad[0]])} vs {int(s1[bad[0]])}"
    assert torch.isfinite(out).all() and torch.isfinite(big).all()
    assert same_bits(out.cpu(), o1.cpu()), first_diff(out.cpu(), o1.cpu())
    assert same_bits(big.cpu(), b1.cpu()), first_diff(big.cpu(), b1.cpu())


# ----------------------------------------------------------------------------------------------- decidable realistic input
@pytest.mark.parametrize("block,extra,seed", [(480, 0, 311), (1920, 333, 312), (9600, 1920, 313)])
def test_realistic_lags_where_fp32_can_decide_them(eng, block, extra, seed):
    """Quasi-periodic input against the fp64 lag.  A case counts only if the fp64 gap between the best and the second-best correlation
    exceeds what a 1920-term fp32 sum can move them by (decidable_bound); the seeds are fixed so that every case counts."""
    n = 24
    y, sola = voiced_case(n, block, extra, seed)
    _o, _b, shift64, corr64 = oracle(y, sola, block, dtype=torch.float64)
    for c in range(n):
        best, gap = gap64(corr64[c])
        assert gap > decidable_bound(sola[c]), f"precondition: case {c} not decidable: gap {gap:.3e} <= {decidable_bound(sola[c]):.3e}"
    assert len(set(shift64)) >= n // 2
    for name, rows in layouts(n):
        _out, _buf, shift = gpu_tail(eng, y[rows], sola[rows], block)
        bad = [(r, int(shift[r]), shift64[c]) for r, c in enumerate(rows) if int(shift[r]) != shift64[c]]
        assert not bad, f"{name}: {len(bad)} lags differ from fp64, (stream, got, fp64): {bad[:5]}"


# ----------------------------------------------------------------------------------------------- phase vocoder
PV_SEEDS = [2, 101, 202, 303, 403, 508, 601, 700, 806, 909]         # one per input, chosen on the CPU so that the preconditions hold
PV_NYQUIST = {8: 0.02, 9: -0.02}                  # inputs with +-0.02 (-1)^j in the buffer and the opposite in the head
PV_LAGS = [0, 241, 700, 960, 1203, 1500, 1686, 1920, 64, 1446]


def pv_input(i, block):
    """(y [Ly], buffer [1920]) of vocoder input i: buffer and head are five harmonics of two different pitches at arbitrary phases
    (0.03 each) over white noise (0.08; half of the head's noise is the buffer's, which is what makes the planted lag decisive).  The
    head sits at PV_LAGS[i] of an otherwise quiet y."""
    g = np.random.default_rng(PV_SEEDS[i])
    t = np.arange(CROSS)

    def harm(f0):
        return sum(0.03 * np.sin(2 * np.pi * f0 * (h + 1) * t / 48000.0 + g.uniform(0, 2 * np.pi)) for h in range(5))

    na, nb = g.standard_normal(CROSS), g.standard_normal(CROSS)
    a = harm(g.uniform(100, 400)) + 0.08 * na
    b = harm(g.uniform(100, 400)) + 0.08 * (0.5 * na + math.sqrt(0.75) * nb)
    if i in PV_NYQUIST:
        a = a + PV_NYQUIST[i] * (-1.0) ** t
        b = b - PV_NYQUIST[i] * (-1.0) ** t
    Ly = block + MIN_LY + 7
    y = torch.from_numpy((0.01 * g.standard_normal(Ly)).astype(np.float32))
    tw = temp_wav(y, block)
    tw[PV_LAGS[i]:PV_LAGS[i] + CROSS] = torch.from_numpy(b.astype(np.float32))
    return y, torch.from_numpy(a.astype(np.float32))


def pv_preconditions(a, b):
    """On the fp64 spectra of the windowed buffer and head: (smallest bin magnitude / largest, smallest distance of dp / 2 pi + 0.5
    from an integer over the bins 1 .. 959).  The wrap is a discontinuity of the formula: a bin that sits on it may legitimately
    land on either side in fp32, so such inputs are not used (bins 0 and 960 are real, and exactly on it when the signs differ:
    there the floor() decides the same way for every exact evaluation, and the Nyquist inputs test precisely that)."""
    w = torch.sqrt((1 - FADE.double()) * FADE.double())
    fa, fb = torch.fft.rfft(a.double() * w), torch.fft.rfft(b.double() * w)
    mags = torch.cat([fa.abs(), fb.abs()])
    x = ((torch.angle(fb) - torch.angle(fa)) / 2 / math.pi + 0.5)[1:-1]
    return float(mags.min() / mags.max()), float((x - torch.round(x)).abs().min())


def test_phase_vocoder_against_fp64(eng):
    """The vocoder head against the fp64 evaluation of the reference's formula.  The yardstick is the reference's own fp32 evaluation
    (one thread): the kernel's direct fp32 DFT and cosine bank may be at most twice as far from the truth, per input.  Both are fp32
    evaluations of one formula that differ in the order of their sums (direct DFT against FFT), so a ratio near 1 is what a correct
    kernel gives (measured on an MI355X: 0.77 ... 0.87 on these ten inputs, errors 1.9e-6 ... 2.2e-6 rms on signals of 0.085 ... 0.09 rms;
    DESIGN.md's error budget); 2 leaves room for that order and none for a wrong twiddle, wrap or scale.
    Everything outside the head is a copy and is compared to the bit."""
    block = 1920
    n = len(PV_SEEDS)
    assert n >= 8
    ins = [pv_input(i, block) for i in range(n)]
    y, sola = torch.stack([p[0] for p in ins]), torch.stack([p[1] for p in ins])
    out64, buf64, shift64, corr64 = oracle(y, sola, block, pv=True, dtype=torch.float64)
    for i in range(n):
        best, gap = gap64(corr64[i])
        assert best == PV_LAGS[i] and gap >= 0.5, f"precondition: input {i}: lag {best}, gap {gap:.3f}"
        floor, wrap = pv_preconditions(sola[i], temp_wav(y[i], block)[best:best + CROSS])
        assert floor >= 1e-3 and wrap >= 1e-3, f"precondition: input {i}: smallest bin {floor:.2e} of the largest, wrap distance {wrap:.2e}"
    with oracle_one_thread():
        out32, buf32, shift32, _c = oracle(y, sola, block, pv=True)
    assert shift32 == PV_LAGS
    out, buf, shift = gpu_tail(eng, y, sola, block, pv=True)
    assert shift.tolist() == PV_LAGS
    assert torch.isfinite(out).all()
    worst = 0.0
    for i in range(n):
        truth = out64[i][:CROSS]
        e_gpu, e_ref = out[i, :CROSS].double() - truth, out32[i][:CROSS].double() - truth
        ratio = rms(e_gpu) / rms(e_ref)
        worst = max(worst, ratio)
        _log(f"[parity] vocoder head input {i}{' (Nyquist)' if i in PV_NYQUIST else ''}: rms err gpu {rms(e_gpu):.3e} oracle-fp32 {rms(e_ref):.3e} "
             f"ratio {ratio:.3f}  max_abs gpu {float(e_gpu.abs().max()):.3e} oracle-fp32 {float(e_ref.abs().max()):.3e}  signal rms {rms(truth):.3e}")
    for i in range(n):
        truth = out64[i][:CROSS]
        e_gpu, e_ref = rms(out[i, :CROSS].double() - truth), rms(out32[i][:CROSS].double() - truth)
        assert e_gpu <= 2 * e_ref, f"input {i}: head rms error {e_gpu:.3e} > 2 x {e_ref:.3e} (the fp32 oracle's)"
        tw = temp_wav(y[i], block)
        assert same_bits(buf[i], tw[PV_LAGS[i] + CROSS:PV_LAGS[i] + 2 * CROSS]), f"input {i}: the buffer is a copy at block = 1920"
        assert same_bits(buf[i], buf32[i])
    _log(f"[parity] vocoder head: worst gpu / oracle-fp32 error ratio {worst:.3f} over {n} inputs (gate 2)")


def test_phase_vocoder_from_the_zero_buffer(eng):
    """Not comparable to the reference: with an all-zero buffer every bin of its spectrum is 0, and atan2 takes its sign from the
    signed zeros the FFT library happens to leave (the formula with pa = 0 is 2.8e-3 from torch's output).  What can be said: the
    lag is 0 (every correlation ties at 0), the output is finite, everything behind the head is a copy, and two runs agree."""
    block = 3840
    y = voiced(3, block + MIN_LY + 333, seed=9)
    sola = torch.zeros(3, CROSS)
    out, buf, shift = gpu_tail(eng, y, sola, block, pv=True)
    out2, buf2, shift2 = gpu_tail(eng, y, sola, block, pv=True)
    assert shift.tolist() == [0, 0, 0] == shift2.tolist()
    assert torch.isfinite(out).all()
    tw = temp_wav(y, block)
    assert same_bits(out[:, CROSS:], tw[:, CROSS:block].contiguous()), "behind the head the block is a copy"
    assert same_bits(buf, tw[:, block:block + CROSS].contiguous()), "at block >= 1920 the next buffer is a copy"
    assert same_bits(out, out2) and same_bits(buf, buf2), "two identical calls differ"


# ----------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_refused_before_any_launch(eng):
    from tinyvc_amd._lib import TinyVCError
    block = 960
    sola = torch.full((2, CROSS), 0.25)
    buf = sola.to(DEV)
    fade = FADE.to(DEV)
    short = torch.zeros(2, block + CROSS + SEARCH + DELAY - 1, device=DEV)
    with pytest.raises(TinyVCError, match="tvc_sola_f32: bad argument"):
        eng.sola(short, buf, fade, block)
    with pytest.raises(TinyVCError, match="tvc_sola_f32: bad argument"):
        eng.sola(torch.zeros(2, 9600, device=DEV), buf, fade, 0)
    torch.cuda.synchronize()
    assert same_bits(buf.cpu(), sola), "a refused call must not touch the buffer"
    # the shortest accepted row
    out = eng.sola(torch.zeros(2, block + CROSS + SEARCH + DELAY, device=DEV), buf, fade, block)
    torch.cuda.synchronize()
    assert out.shape == (2, block)


# ----------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("S", [3, S_ONE_WG])
@pytest.mark.parametrize("where", ["buffer", "y"])
def test_a_nan_stream_gets_the_oracles_lag_and_leaves_the_others_alone(eng, S, where):
    """One NaN in the buffer of a stream makes every correlation of that stream NaN; one in y makes a run of lags NaN.  torch.argmax
    returns the first NaN, and so must the kernels' arg-max (lag_ahead in sola.hip) on both branches; the lag stays in [0, 1920]
    whatever the values are, because the tail indexes y with it.  The other streams do not notice."""
    block = 960
    y3, sola3 = voiced_case(3, block, 333, seed=55)
    rows = [r % 3 for r in range(S)]
    y, sola = y3[rows].clone(), sola3[rows].clone()
    hit = [1] if S == 3 else [1, 4, S - 1]          # streams of case 1
    assert all(rows[h] == 1 for h in hit)
    clean = gpu_tail(eng, y, sola, block)
    for h in hit:
        if where == "buffer":
            sola[h, 1234] = float("nan")
        else:
            temp_wav(y, block)[h, 2500] = float("nan")       # lags 581 .. 1920 cover it
    with oracle_one_thread():
        _o, _b, ref_shift, ref_corr = oracle(y[hit[:1]], sola[hit[:1]], block)
    want = ref_shift[0]
    assert want == (0 if where == "buffer" else 2500 - CROSS + 1) and bool(torch.isnan(ref_corr[0][want]))
    out, buf, shift = gpu_tail(eng, y, sola, block)
    assert int(shift.min()) >= 0 and int(shift.max()) <= SEARCH
    assert [int(shift[h]) for h in hit] == [want] * len(hit)
    keep = torch.ones(S, dtype=torch.bool)
    keep[hit] = False
    assert torch.equal(shift[keep], clean[2][keep])
    assert same_bits(out[keep], clean[0][keep]) and same_bits(buf[keep], clean[1][keep])
