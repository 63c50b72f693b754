"""Shared test helpers: golden fixture loading and formula-regenerated inputs."""
import os

import numpy as np
import torch

from tinyvc_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def convert_inputs(g):
    """Inputs of a `convert_*` fixture, rebuilt from the seeds it records."""
    wf = synth.synth_wave(int(g["batch"]), int(g["wave_len"]), seed=int(g["wave_seed"]))
    tgt = synth.synth_index(int(g["index_size"]), seed=int(g["index_seed"]))
    frames = g["wave"].shape[1] // 480
    angle = synth.synth_angle(int(g["batch"]), frames, int(g["noise_seed"]))
    return wf, tgt, float(g["pitch_shift"]), angle


class oracle_one_thread:
    """The oracle's waveform depends on the host's thread count (oneDNN / MKL reduction orders: 2e-4 rms between 1 and 128
    threads at T = 200 on the GPU box's host).  Live comparisons run it on ONE thread - sequential
    reductions, the reproducible setting (the committed fixtures came from the 8-thread build host)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


_SD = {}


def state_dicts(seed=0):
    if seed not in _SD:
        _SD[seed] = (synth.synth_state_dict("encoder", seed), synth.synth_state_dict("decoder", seed))
    return _SD[seed]


def rms(a):
    a = torch.as_tensor(a).double()
    return float(torch.sqrt((a * a).mean()))


def rel_rms(a, ref):
    return rms(torch.as_tensor(a).double() - torch.as_tensor(ref).double()) / max(rms(ref), 1e-30)


def window_starts(n, width=32):
    """First columns of the windows `window_errors` measures on a length-n axis: `width` columns every `width // 2`, plus one window
    that ends on the last column; one window over everything when n <= width."""
    if n <= width:
        return [0]
    starts = list(range(0, n - width + 1, max(width // 2, 1)))
    if starts[-1] != n - width:
        starts.append(n - width)
    return starts


def window_errors(x, truth, width=32):
    """[B, C, len] against an fp64 `truth` -> [B, windows] (fp64): per row b and window (window_starts), the rms over (C, window) of
    x - truth divided by the rms of truth[b] over the WHOLE row.  A whole-tensor relative rms dilutes an error confined to the last columns
    of a tile by sqrt(columns / len) (1e-4 in two of 3096 columns reads 2.5e-6); here those columns sit in a full-width window of their own."""
    truth = torch.as_tensor(truth)
    assert truth.dtype == torch.float64 and truth.dim() == 3 and tuple(x.shape) == tuple(truth.shape)
    d = torch.as_tensor(x).double() - truth
    B, C, n = truth.shape
    cs = torch.cat([torch.zeros(B, 1, dtype=torch.float64), (d * d).sum(dim=1).cumsum(dim=1)], dim=1)      # [B, n + 1]
    st = torch.tensor(window_starts(n, width))
    w = min(width, n)
    num = torch.sqrt((cs[:, st + w] - cs[:, st]).clamp_min(0.0) / (C * w))
    den = torch.sqrt((truth * truth).mean(dim=(1, 2))).clamp_min(1e-30)
    return num / den[:, None]


def stage(g, name):
    """(tensor, time stride) of a stored stage output.  Round-1 fixtures keep the encoder-side tensors whole and
    decimate the full-rate ones by `decim`; the headline-length fixtures (convert_cfg*) store `<name>_d` with its own
    `<name>_stride` (tools/gen_golden.py)."""
    if name in g:
        return torch.from_numpy(np.asarray(g[name])), 1
    if name + "_stride" in g:
        return torch.from_numpy(np.asarray(g[name + "_d"])), int(g[name + "_stride"])
    dm = int(g["decim"])
    if name.startswith("skip"):
        st = dm if int(name[4:]) < 2 else 1
    elif name.startswith("up"):
        st = dm if int(name[2:]) >= 3 else 1
    else:
        st = dm
    return torch.from_numpy(np.asarray(g[name + "_d"])), st


# ---- front end, pitch decode and DSP edge cases (test_gpu_front_dsp_edges.py, test_front_dsp_metric_host.py) ----------------------------
def frame_bin_errors(x, truth):
    """[B, 961, T] against an fp64 `truth` -> (per frame [B, T], per bin [B, 961]), fp64.  Per frame t: the rms over bins of x - truth divided by
    the rms of the WHOLE row.  Per bin k: the rms over frames of x - truth divided by the rms over frames of truth at that bin - the bin's own
    scale, so a bin far below the row's loudest (bin 960 of a low-passed signal) is not hidden by them."""
    truth = torch.as_tensor(truth)
    assert truth.dtype == torch.float64 and truth.dim() == 3 and tuple(x.shape) == tuple(truth.shape)
    d2 = (torch.as_tensor(x).double() - truth) ** 2
    row = torch.sqrt((truth * truth).mean(dim=(1, 2))).clamp_min(1e-300)
    per_frame = torch.sqrt(d2.mean(dim=1)) / row[:, None]
    per_bin = torch.sqrt(d2.mean(dim=2)) / torch.sqrt((truth * truth).mean(dim=2)).clamp_min(1e-300)
    return per_frame, per_bin


def frame_element_errors(x, truth, frame=480):
    """[B, L] against an fp64 `truth` -> (per frame [B, L / frame], per element [B, L]), both relative to the row's rms.  Samples where the
    truth is NaN count nowhere: not in the row's rms, not in a frame's mean (a frame of NaNs reads 0), and their element error is 0."""
    truth = torch.as_tensor(truth)
    assert truth.dtype == torch.float64 and truth.dim() == 2 and tuple(x.shape) == tuple(truth.shape) and truth.shape[1] % frame == 0
    ok = ~torch.isnan(truth)
    t0 = torch.where(ok, truth, torch.zeros_like(truth))
    d = torch.where(ok, torch.as_tensor(x).double() - t0, torch.zeros_like(truth))
    n_row = ok.sum(dim=1).clamp_min(1)
    row = torch.sqrt((t0 * t0).sum(dim=1) / n_row).clamp_min(1e-300)
    B = truth.shape[0]
    n_fr = ok.view(B, -1, frame).sum(dim=2).clamp_min(1)
    per_frame = torch.sqrt((d * d).view(B, -1, frame).sum(dim=2) / n_fr) / row[:, None]
    return per_frame, d.abs() / row[:, None]


def decidable_samples(inc, margin):
    """The oscillator's decidable samples.  inc: the oracle's fp32 phase increments of one (utterance, harmonic), 1-D.  The oracle's phase is
    P = their sequential fp64 sum, rounded to fp32 (I).  Where P lies more than `margin` (cycles; a number or one per sample) from both
    rounding midpoints of I, every summation order whose drift stays within the margin gives the same I, hence the same sample up to the
    sine's last bit -> (decidable [n] bool, P fp64, I fp32)."""
    P = np.cumsum(np.asarray(inc, dtype=np.float32).reshape(-1).astype(np.float64))
    I = P.astype(np.float32)
    lo = (I.astype(np.float64) + np.nextafter(I, np.float32(-np.inf)).astype(np.float64)) / 2
    hi = (I.astype(np.float64) + np.nextafter(I, np.float32(np.inf)).astype(np.float64)) / 2
    return np.minimum(P - lo, hi - P) > margin, P, I


def summation_order_margin(P):
    """The margin of decidable_samples for short utterances: 4 (i + 1) 2^-53 P_i.  Any order of adding i + 1 positive fp64 terms lies within
    (i + 1) 2^-53 P_i of the sequential sum (every partial sum is at most P_i, every addition rounds by at most 2^-53 of it); the factor 4
    covers the oracle's own sequential roundings and the kernels' three-level scan together."""
    P = np.asarray(P, dtype=np.float64)
    return 4.0 * np.arange(1, P.shape[0] + 1, dtype=np.float64) * 2.0 ** -53 * P


def sums_exact_in_any_order(inc):
    """True where NO fp64 addition of these fp32 increments can round, in whatever order and grouping they are added: all of them are whole
    multiples of q = the lowest set bit among them, so is every partial sum, and a multiple of q below 2^53 q is an fp64 number.  The drift
    between two summation orders is then 0, not (i + 1) 2^-53 P_i.  It matters at these lengths: under a constant f0 the phase is
    P_i = (i + 1) c exactly, which IS a rounding midpoint of fp32 for a few per cent of the i (3 c has 25 or 26 significant bits) - and both
    sides round that tie to even.  A margin rule alone would call those samples, and every sample of an unvoiced tail that stands on one,
    non-decidable."""
    bits = np.asarray(inc, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.int64)
    exp, man = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    nz = (exp | man) != 0
    if not nz.any():
        return True
    man = np.where(exp > 0, man | 0x800000, man)[nz]
    e = np.maximum(exp[nz], 1) - 150                                          # value = man * 2^e
    low = e + np.log2((man & -man).astype(np.float64)).astype(np.int64)       # exponent of the lowest set bit
    total = float(np.asarray(inc, dtype=np.float64).sum())
    return total < 2.0 ** (53 + int(low.min()))


def decidable_short(inc):
    """decidable_samples for the short utterances of test_gpu_front_dsp_edges.py: every sample where the sums are exact in any order,
    else those further than summation_order_margin from a rounding midpoint -> (decidable, P, I)."""
    _d, P, _I = decidable_samples(inc, 0.0)
    dec, P, I = decidable_samples(inc, summation_order_margin(P))
    if sums_exact_in_any_order(inc):
        dec = np.ones_like(dec)
    return dec, P, I


def decode_lower_id_first(logits):
    """PitchEstimator.decode restated with the kernels' tie rule (ties go to the lower class id): a stable descending sort, its first four
    entries, softmax, the class frequencies 20 * 2^(id / 48) with the oracle's '<= 20 Hz -> 0' rule, the output gate.  Every operation after
    the sort is the oracle's own (oracle.ref_cpu.pitch_decode), in its order and in the dtype of `logits` -> (f0 [B, 1, T], the value in
    front of the output gate [B, 1, T], the four class ids [B, 4, T], tie_free [B, T]: the first five sorted logits strictly decrease)."""
    import torch.nn.functional as F
    srt = torch.sort(logits, dim=1, descending=True, stable=True)
    top, ids = srt.values[:, :4], srt.indices[:, :4]
    p = F.softmax(top, dim=1)
    fr = 20.0 * (2 ** (ids.to(logits.dtype) / 48))
    fr = torch.where(fr <= 20.0, torch.zeros_like(fr), fr)
    raw = (p * fr).sum(dim=1, keepdim=True)
    f0 = torch.where(raw <= 20.0, torch.zeros_like(raw), raw)
    tie_free = (srt.values[:, :4] > srt.values[:, 1:5]).all(dim=1)
    return f0, raw, ids, tie_free


# the inputs of those two files, a function of the shape alone (both files, and both machines, build the same tensors)
STFT_SHAPES = [(1, 3), (2, 4), (1, 7), (2, 8), (3, 9), (2, 12), (1, 17)]
# the per-bin gate's factor over the oracle's worst bin: 2, except where a case is listed with its measured figures and the reason
# (module docstring of test_gpu_front_dsp_edges.py, item 1); never above 4
STFT_BIN_FACTOR = {(1, 3, "synth"): 4.0}
ENERGY_LENGTHS = [128, 129, 191, 192, 193, 1437, 1438, 1439, 1440, 61920, 61921]
DECODE_SHAPES = [(1, 1), (3, 21), (1, 64), (5, 13), (3, 43)]                  # B * T = 1, 63, 64, 65, 129
DSP_SHAPES = [(1, 1), (2, 2), (1, 3), (3, 5), (2, 9), (1, 17)]
F0_PATTERNS = ["unvoiced_first", "unvoiced_last", "voiced_first_only", "voiced_last_only", "exactly_20", "just_above_20", "all_zero", "800_hz"]


def stft_edge_wave(kind, B, T):
    """[B, 480 T].  'synth': synth.synth_wave (its first 1200 samples are silent).  'spikes': white noise with large isolated samples at
    0, 1, L - 2 and L - 1, all four different, so that a reflection off by one sample changes the three frames that reflect."""
    L = 480 * T
    if kind == "synth":
        return synth.synth_wave(B, L, seed=3000 + T)
    g = torch.Generator().manual_seed(3100 + T)
    wf = 0.1 * torch.randn(B, L, generator=g)
    wf[:, 0], wf[:, 1], wf[:, L - 2], wf[:, L - 1] = 1.5, -2.0, 1.75, -1.25
    return wf


def energy_edge_wave(B, L):
    g = torch.Generator().manual_seed(5000 + L)
    wf = 0.3 * torch.randn(B, L, generator=g)
    wf[:, 0] = -0.8
    wf[:, L - 1] = 1.0 + 0.1 * torch.arange(B)
    return wf


def _decode_columns():
    """name -> f(generator) -> [512] logits of one column"""
    ids = torch.arange(512.0)

    def prior(g):      # the synthetic checkpoint's prior: a parabola centred on class 150
        return -2.0 * ((ids - 150.0) / 30.0) ** 2 + torch.randn(512, generator=g)

    def low(g):
        return -30.0 + torch.randn(512, generator=g)

    def put(col, pairs):
        for i, v in pairs:
            col[i] = v
        return col

    def class0(g):     # class 0 (0 Hz) wins on part of the frames, as in the checkpoint
        c = prior(g)
        c[0] = c.max() + 1.0 + torch.rand(1, generator=g)[0]
        return c

    def best_511(g):
        c = prior(g)
        c[511] = c.max() + 2.0
        return c

    return {
        "prior": prior,
        "prior_class0": class0,
        "tie_top_31_32": lambda g: put(low(g), [(31, 5.0), (32, 5.0), (100, 3.0), (200, 2.5)]),            # waves 0 | 1, both inside the top four
        "tie_top_5_500": lambda g: put(low(g), [(500, 4.0), (5, 4.0), (250, 3.5), (251, 1.0)]),             # waves 0 | 15
        "tie_4th_31_32": lambda g: put(low(g), [(100, 5.0), (200, 4.0), (300, 3.0), (32, 2.0), (31, 2.0)]),  # 31 is in, 32 is out
        "tie_4th_5_500": lambda g: put(low(g), [(150, 5.0), (160, 4.5), (170, 4.0), (500, 3.25), (5, 3.25)]),
        "tie_4th_three_way": lambda g: put(low(g), [(10, 3.0), (20, 2.5), (30, 2.0), (447, 1.0), (64, 1.0), (63, 1.0)]),      # waves 13 | 2 | 1: 63 is in
        "all_equal": lambda g: torch.full((512,), 1.25),                                                    # classes 0 .. 3: 15.4 Hz, below the gate
        "four_waves": lambda g: put(low(g), [(10, 4.0), (170, 3.5), (300, 3.0), (511, 2.5)]),               # waves 0, 5, 9, 15
        "class0_alone": lambda g: put(-200.0 + torch.randn(512, generator=g), [(0, 10.0)]),                 # exactly 0
        "best_511": best_511,
        "two_finite": lambda g: put(torch.full((512,), float("-inf")), [(40, 1.0), (41, 0.5)]),
        "two_finite_tied": lambda g: put(torch.full((512,), float("-inf")), [(480, 0.3), (7, 0.3)]),
    }


DECODE_SPECIALS = [k for k in _decode_columns() if not k.startswith("prior")]


def decode_edge_logits(B, T, rot=0):
    """([B, 512, T] fp32 logits, the column kinds in column order n = b T + t).  The first and the last len(DECODE_SPECIALS) columns are the
    constructed ones, rotated by `rot` - the last workgroup's few columns (n = 64, n = 128) get them too -, the columns between are
    prior-shaped random ones, every third with class 0 in front."""
    cols, n, K = _decode_columns(), B * T, len(DECODE_SPECIALS)
    g = torch.Generator().manual_seed(6000 + 7 * n + rot)
    out, kinds = torch.empty(n, 512), []
    for c in range(n):
        if c < K or c >= n - K:
            kind = DECODE_SPECIALS[(c + rot) % K]
        else:
            kind = "prior_class0" if c % 3 == 0 else "prior"
        kinds.append(kind)
        out[c] = cols[kind](g)
    return out.view(B, T, 512).transpose(1, 2).contiguous(), kinds


def dsp_edge_inputs(B, T):
    """(amps [B, 15, T], kernel [B, 961, T], phases [B, 961, T] in [-pi, pi))"""
    g = torch.Generator().manual_seed(4000 + T)
    amps = 0.05 + 2.0 * torch.rand(B, 15, T, generator=g)
    kern = 0.05 + torch.rand(B, 961, T, generator=g)
    return amps, kern, synth.synth_angle(B, T, 4100 + T)


def dsp_edge_f0(pattern, B, T):
    """[B, 1, T] f0 as pitch_decode emits it (0 = unvoiced, else above 20 Hz), and the gate's own edge: exactly 20.0 is unvoiced, the next
    float is voiced."""
    g = torch.Generator().manual_seed(4200 + T)
    base = 60.0 + 440.0 * torch.rand(B, 1, T, generator=g)
    f0 = base.clone()
    if pattern == "unvoiced_first":
        f0[..., 0] = 0.0
    elif pattern == "unvoiced_last":
        f0[..., -1] = 0.0
    elif pattern == "voiced_first_only":
        f0 = torch.zeros_like(base)
        f0[..., 0] = base[..., 0]
    elif pattern == "voiced_last_only":
        f0 = torch.zeros_like(base)
        f0[..., -1] = base[..., -1]
    elif pattern == "exactly_20":
        f0[..., ::2] = 20.0
    elif pattern == "just_above_20":
        f0[..., ::2] = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))
    elif pattern == "all_zero":
        f0 = torch.zeros_like(base)
    elif pattern == "800_hz":
        f0 = torch.full_like(base, 800.0)
    else:
        raise ValueError(pattern)
    return f0


def harmonic_increments(f0):
    """The oracle's phase increments, op for op (oracle.ref_cpu.oscillate_harmonics): [B, 15, 480 T] fp32."""
    import torch.nn.functional as F
    mul = (torch.arange(15) + 1).view(1, -1, 1)
    return (F.interpolate(f0, f0.shape[2] * 480, mode="linear") * mul) / 24000


# ---- window and row gates at tile edges (test_gpu_tile_edges.py, test_gpu_contraction_edges.py, test_contraction_metric_host.py) ---------
FLOOR = 3e-6


def _group(name):
    return name.split("[")[0]


def _gate_case(case, gpu, truth, ref, extra=""):
    """gpu / truth / ref: {name: [rows, C, len]} (gpu on the host).  Logs the case's `[edge]` line; returns (failures, {name: [rows] gates})."""
    fails, gates, ermax, groups = [], {}, {}, {}
    worst = None                                      # (e / gate, e, gate, name, row, column)
    for name, t in truth.items():
        g = gpu[name].cpu()
        assert torch.isfinite(g).all(), f"{case} {name}: non-finite"
        eg, er = window_errors(g, t), window_errors(ref[name], t)
        gate = (2.0 * er.max(dim=1).values).clamp_min(FLOOR)
        gates[name], ermax[name] = gate, er.max(dim=1).values
        st = window_starts(t.shape[2])
        a, b = groups.get(_group(name), (0.0, 0.0))
        groups[_group(name)] = (max(a, float(eg.max())), max(b, float(er.max())))
        ratio = eg / gate[:, None]
        r, w = divmod(int(ratio.argmax()), ratio.shape[1])
        if worst is None or float(ratio[r, w]) > worst[0]:
            worst = (float(ratio[r, w]), float(eg[r, w]), float(gate[r]), name, r, st[w])
        for r, w in (ratio > 1.0).nonzero().tolist()[:4]:
            fails.append(f"{name} row {r} columns [{st[w]}, {st[w] + min(32, t.shape[2])}) of {t.shape[2]}: {float(eg[r, w]):.2e} > gate {float(gate[r]):.2e}")
    _x, e, gt, name, r, col = worst
    print(f"[edge] {case}: worst window GPU {e:.2e} (gate {gt:.2e}, oracle fp32 worst {float(ermax[name][r]):.2e}) "
          f"at {name} row {r} column {col} of {truth[name].shape[2]}; whole tensor {rel_rms(gpu[name].cpu(), truth[name]):.2e}; worst GPU / oracle window per group: "
          + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in groups.items()) + extra)
    return fails, gates


def _bump_trips(gpu, truth, gates, name):
    """The gate's own sensitivity: + 1e-4 x rms on the last two columns of block `name`, on the host; does a window exceed its gate?"""
    t = truth[name]
    bumped = gpu[name].cpu().double().clone()
    bumped[..., -2:] += 1e-4 * torch.sqrt((t * t).mean(dim=(1, 2)))[:, None, None]
    return bool((window_errors(bumped, t) > gates[name][:, None]).any())


# FilterNet cases of test_gpu_tile_edges.py (a) and (b); test_wave_truth_host.py proves their truth and gates with the oracle alone
FILTER_EDGE_LENGTHS = [1, 3, 9, 12, 25, 26, 28, 37, 43, 65, 127, 128, 129, 136, 512]       # (a): B = 1; the seam table is in the GPU file
WIDE_FILM_SHAPES = [(64, 100), (256, 5)]                                                   # (b): (B, T), rows 0, 1, B / 2, B - 1
_SD64 = {}


def sd64():
    """(encoder, decoder) state_dicts(0) in fp64"""
    if not _SD64:
        enc_sd, dec_sd = state_dicts(0)
        _SD64["e"] = {k: v.double() for k, v in enc_sd.items()}
        _SD64["d"] = {k: v.double() for k, v in dec_sd.items()}
    return _SD64["e"], _SD64["d"]


def filter_edge_inputs(B, T):
    """test_filter_net_blocks_out_of_range's recipe at scale 1, seed 1000 + T -> (content, f0, energy, source)."""
    g = torch.Generator().manual_seed(1000 + T)
    L = 480 * T
    content = torch.randn(B, 768, T, generator=g) * 0.5
    f0 = 80.0 + 200.0 * torch.rand(B, 1, T, generator=g)
    source = torch.randn(B, 16, L, generator=g) * 0.3
    energy = torch.rand(B, 1, L, generator=g)
    return content, f0, energy, source


def filter_named(wave, skips, ups):
    """filter_net's (waveform, skips, ups) -> the ten compared tensors by name; ups[4] is not among them: the waveform is its only view."""
    d = {f"downs[{i}]": s for i, s in enumerate(skips)}
    d.update({f"ups[{i}]": u for i, u in enumerate(ups[:4])})
    d["wave"] = wave if wave.dim() == 3 else wave[:, None, :]
    return d


def filter_edge_oracle(inputs, fp32_positions=True):
    """(truth, yardstick) of the ten compared tensors for the given rows.  Truth: the oracle in fp64 at the source positions ATen computes
    for fp32 tensors (oracle.ref_cpu.fp32_positions); fp32_positions=False: at fp64 positions, the truth of test_gpu_truth.py.  Yardstick:
    the oracle in fp32 on one thread."""
    import contextlib

    from oracle import ref_cpu as R
    _e64, d64 = sd64()
    _enc_sd, dec_sd = state_dicts(0)
    with R.fp32_positions() if fp32_positions else contextlib.nullcontext():
        truth = filter_named(*R.filter_net(d64, *[x.double() for x in inputs], return_blocks=True))
    with oracle_one_thread():
        ref = filter_named(*R.filter_net(dec_sd, *inputs, return_blocks=True))
    return truth, ref


def row_errors(x, truth):
    """[B, C, len] against an fp64 `truth` -> [B, C] (fp64): per utterance b and output row c, the rms over time of x - truth divided by the rms
    of truth[b] over the WHOLE utterance - window_errors with rows for columns.  Not the row's own rms: ELU + 1 outputs go down to 5e-6 where
    the pre-activation is very negative, and there the fp32 oracle itself reads 5e-3 on the row's scale (1e-7 in the utterance's units)."""
    return window_errors(torch.as_tensor(x).transpose(1, 2), torch.as_tensor(truth).transpose(1, 2), width=1)


# SourceNet (B, T): see the table in test_gpu_contraction_edges.py; the two cases that also carry the planted errors on the GPU
SOURCE_SHAPES = [(1, 1), (1, 3), (3, 32), (3, 33), (3, 43), (2, 64), (2, 65), (1, 127), (1, 128), (1, 129), (1, 1024), (1, 1025)]
SOURCE_BUMP_SHAPES = [(3, 43), (1, 129)]


def sourcenet_edge_inputs(B, T, seed=None):
    """(content [B, 768, T], f0 [B, 1, T], energy [B, 1, 480 T]) for SourceNet.  f0: every third frame exactly 0 and the last frame -5.0 - the
    relu and log(1e-6) branches of the f0 conditioning.  energy: each frame's maximum planted alternately on sample 0 and on sample 479 of
    the frame - the first and the last load of the frame-maximum kernel; every other sample is below 1."""
    g = torch.Generator().manual_seed(7000 + 131 * B + T if seed is None else seed)
    content = 0.5 * torch.randn(B, 768, T, generator=g)
    f0 = 80.0 + 200.0 * torch.rand(B, 1, T, generator=g)
    f0[..., ::3] = 0.0
    f0[..., -1] = -5.0
    energy = torch.rand(B, 1, 480 * T, generator=g)
    peak = 1.0 + 0.5 * torch.rand(B, T, generator=g)
    fr = energy.view(B, T, 480)
    fr[:, 0::2, 0] = peak[:, 0::2]
    fr[:, 1::2, 479] = peak[:, 1::2]
    return content, f0, energy


CONVNEXT_LAYERS = {"ssl_feature_estimator": 6, "pitch_estimator": 4, "source_net": 3}          # trunk -> its ConvNeXt layers (mid_layers.i)


def convnext_prefixes(trunks, which="all"):
    """The state-dict prefixes of the ConvNeXt layers of `trunks`; which = 'all', or 'second': every second layer (mid_layers.1, .3, .5)."""
    return [f"{t}.mid_layers.{i}" for t in trunks for i in range(CONVNEXT_LAYERS[t]) if which == "all" or i % 2 == 1]


def rescaled_ln(sd, prefixes, k=12):
    """A copy of `sd` with norm.gamma and norm.beta x 2^k and c2.weight x 2^-k for the named ConvNeXt layers: the same function exactly
    (powers of two; LayerNorm's output and every product of the 1x1 behind it scale without rounding), but the layer's LayerNorm bound
    (ln_bound) grows by 2^k."""
    out = dict(sd)
    for p in prefixes:
        out[p + ".norm.gamma"] = sd[p + ".norm.gamma"] * 2.0 ** k
        out[p + ".norm.beta"] = sd[p + ".norm.beta"] * 2.0 ** k
        out[p + ".c2.weight"] = sd[p + ".c2.weight"] * 2.0 ** -k
    return out


def ln_bound(sd, prefix):
    """pack.hip's bound on a ConvNeXt layer's LayerNorm output, restated in fp32: sqrt(C) max|gamma| + max|beta|.  At 32768 and above the
    fused ConvNeXt launches refuse the layer and the five unfused launches run it, with a |max| slot on the first 1x1's input."""
    g, b = sd[prefix + ".norm.gamma"].float(), sd[prefix + ".norm.beta"].float()
    return float(np.float32(np.sqrt(np.float32(g.numel()))) * np.float32(g.abs().max()) + np.float32(b.abs().max()))


def gemm_s2_width(ncols, mblocks, ncu):
    """gemm_s2_try's column-tile width rule restated (the width in units of 32 columns, 2 .. 6): the fewest rounds of the chip's persistent
    workgroups (one per CU, a multiple of 8) times (width + 64 columns of staging); the narrower tile on a tie.  Used to CHOOSE and ASSERT
    test shapes only."""
    slots = ncu // 8 * 8
    best, best_cost = None, None
    for nwv in range(2, 7):
        tiles = -(-ncols // (nwv * 32)) * mblocks
        cost = -(-tiles // slots) * (nwv * 32 + 64)
        if best_cost is None or cost < best_cost:
            best, best_cost = nwv, cost
    return best


SSL_OUT_MBLOCKS, PIT_OUT_MBLOCKS = 6, 4                          # 768 and 512 output rows in blocks of 128
WIDE_SHAPES_256 = [(3, 897), (17, 241), (3, 1814), (2, 3361)]    # (B, T): ssl_out widths 3, 4, 5, 6 on 256 CUs, tails of 3, 1, 2, 2 columns


def wide_tile_shapes(ncu, span=400):
    """[(B, T)] x 4: for ssl_out widths 3, 4, 5, 6 on a chip of `ncu` CUs, the T nearest to WIDE_SHAPES_256's at which B T selects that width and
    leaves a tail of 1 .. 3 columns behind the last full tile; None where no T within `span` does."""
    out = []
    for want, (B, T0) in zip((3, 4, 5, 6), WIDE_SHAPES_256):
        pick = None
        for d in range(span + 1):
            for T in ((T0,) if d == 0 else (T0 - d, T0 + d)):
                if pick is None and T >= 3 and gemm_s2_width(B * T, SSL_OUT_MBLOCKS, ncu) == want and 1 <= (B * T) % (32 * want) <= 3:
                    pick = (B, T)
        out.append(pick)
    return out


def edge_gate(e_ref):
    """The rule of the tile-edge files for one case, tensor and metric: max(3e-6, 2 x the oracle's own worst figure)."""
    return max(FLOOR, 2.0 * float(e_ref.max()))


_METRICS = (("window", window_errors, window_starts), ("row", row_errors, None))


def gate_windows_and_rows(case, x, truth, ref, extra="", log=True):
    """x / truth / ref: {name: [B, C, len]}.  Every tensor under both metrics - 32-column windows and output rows - against
    edge_gate(the oracle's fp32 figures of this case, tensor and metric).  Logs the case's `[edge]` line -> (failures, {(name, metric): gate})."""
    fails, gates, parts = [], {}, []
    for name, t in truth.items():
        g = torch.as_tensor(x[name]).cpu()
        assert torch.isfinite(g).all(), f"{case} {name}: non-finite"
        for metric, fn, starts in _METRICS:
            eg, er = fn(g, t), fn(ref[name], t)
            gate = gates[name, metric] = edge_gate(er)
            b, i = divmod(int(eg.argmax()), eg.shape[1])
            where = f"row {i}" if starts is None else f"column {starts(t.shape[2])[i]} of {t.shape[2]}"
            parts.append(f"{name} per {metric} GPU {float(eg.max()):.2e} (utterance {b} {where}) / oracle fp32 {float(er.max()):.2e} / gate {gate:.2e}")
            for b, i in (eg > gate).nonzero().tolist()[:4]:
                where = f"row {i}" if starts is None else f"columns from {starts(t.shape[2])[i]} of {t.shape[2]}"
                fails.append(f"{name} utterance {b} {where}: {float(eg[b, i]):.2e} > gate {gate:.2e}")
    if log:
        print(f"[edge] {case}: " + "; ".join(parts) + "; whole tensor " + ", ".join(f"{k} {rel_rms(torch.as_tensor(x[k]).cpu(), t):.2e}" for k, t in truth.items()) + extra)
    return fails, gates


def planted_errors_trip(x, truth, gates):
    """The gates' own sensitivity, on the host -> the planted errors that did NOT trip their gate (want: none).  `kernel` row 960 and
    `amps` row 14 x (1 + 1e-4) against the row gate; + 1e-4 x the utterance's rms on the last two columns of each tensor against the window gate."""
    missed = []
    for name, row in (("kernel", 960), ("amps", 14)):
        b = torch.as_tensor(x[name]).cpu().double().clone()
        b[:, row] *= 1.0 + 1e-4
        if not bool((row_errors(b, truth[name])[:, row] > gates[name, "row"]).all()):
            missed.append(f"{name} row {row} x (1 + 1e-4)")
    for name, t in truth.items():
        b = torch.as_tensor(x[name]).cpu().double().clone()
        b[..., -2:] += 1e-4 * torch.sqrt((t * t).mean(dim=(1, 2)))[:, None, None]
        if not bool((window_errors(b, t)[:, -1] > gates[name, "window"]).all()):
            missed.append(f"{name} last two columns + 1e-4 x rms")
    return missed
