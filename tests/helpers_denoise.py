"""The definition of the streams' spectral suppressor (tvc_stream_denoise_f32, include/tinyvc_hip.h) restated on the CPU, shared by
tests/test_stream_denoise_host.py and tests/test_gpu_stream_denoise.py.  `Restated` evaluates it in fp64 - the reference - or, with
dtype=torch.float32, in fp32 with torch.fft in float32 - the yardstick an fp32 kernel's error is held against.  Both take the host's fp32
scalars (a_s, a_n, clamp, beta: module.infer.stream.denoise_constants) widened, not recomputed.  The window is the definition's, made in
fp64: the reference keeps it so (the overlap-add of its square is 1 to the last place), the yardstick rounds it to fp32 once, as the
kernel's table is."""
import math

import numpy as np
import torch

NF, BINS = 640, 321
NMIN, TINY = 1e-12, 1e-30
# w[n] = sqrt(0.5 - 0.5 cos(2 pi n / 640)), tabulated in fp64
WINDOW = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NF) / NF))
_BIN_WEIGHT = np.full(BINS, 2.0)
_BIN_WEIGHT[0] = _BIN_WEIGHT[-1] = 1.0


class Restated:
    """One stream.  run(block, reduction_db) -> the block's output; hist, ola, smooth, noise, frames are the state after it."""

    def __init__(self, hop, a_s, a_n, clamp, beta, warm, dtype=torch.float64):
        assert hop in (160, 320)
        self.hop, self.D, self.dtype = hop, NF - hop, dtype
        self.a_s, self.a_n, self.clamp, self.beta, self.warm = float(a_s), float(a_n), float(clamp), float(beta), int(warm)
        self.w = torch.from_numpy(WINDOW).to(dtype)
        self.scale = 2.0 * hop / NF
        self.hist = torch.zeros(self.D, dtype=dtype)
        self.ola = torch.zeros(self.D, dtype=dtype)
        self.smooth = torch.zeros(BINS, dtype=dtype)
        self.noise = torch.zeros(BINS, dtype=dtype)
        self.frames = 0

    def run(self, x, reduction_db):
        dt, hop = self.dtype, self.hop
        x = torch.from_numpy(np.array(x)).to(dt)
        n = x.numel()
        assert n >= hop and n % hop == 0
        floor = float(torch.tensor(10.0, dtype=dt) ** torch.tensor(-max(float(reduction_db), 0.0) / 20.0, dtype=dt))
        seq = torch.cat([self.hist, x])
        acc = torch.cat([self.ola, torch.zeros(n, dtype=dt)])
        for m in range(n // hop):
            f = seq[m * hop:m * hop + NF]
            if not bool((f != 0).any()):      # +-0 only: nothing is added, nothing moves
                continue
            X = torch.fft.rfft(self.w * f)
            P = X.real ** 2 + X.imag ** 2
            self.smooth = self.a_s * self.smooth + (1.0 - self.a_s) * P
            if self.frames < self.warm:
                self.noise = self.noise + (P - self.noise) / (self.frames + 1)
            else:
                self.noise = self.a_n * self.noise + (1.0 - self.a_n) * torch.minimum(P, torch.clamp(self.clamp * self.noise, min=NMIN))
            G = torch.clamp(1.0 - self.beta * self.noise / torch.clamp(self.smooth, min=TINY), min=floor)
            y = torch.fft.irfft(G * X, n=NF)
            acc[m * hop:m * hop + NF] += y * self.w * self.scale      # ascending frame order onto the carried tail
            self.frames = min(self.frames + 1, 2 ** 30)
        self.hist = seq[n:].clone()
        self.ola = acc[n:].clone()
        return acc[:n].clone()

    def noise_db(self):
        s = float((self.noise.double().numpy() * _BIN_WEIGHT).sum()) / (NF * (NF // 2))
        return 10.0 * math.log10(max(s, 1e-20))


def run_stream(x, block, reduction_db, constants, hop, dtype=torch.float64):
    """a whole signal in blocks of `block` -> (output, the Restated after the last block)"""
    r = Restated(hop, *constants, dtype=dtype)
    x = np.asarray(x)
    assert len(x) % block == 0
    out = [r.run(x[i:i + block], reduction_db) for i in range(0, len(x), block)]
    return torch.cat(out), r


# ---- the behaviour the issue states for the definition ----------------------------------------------------------------------------------------
BEHAVIOUR = dict(reduction_db=18.0, strength=2.0, clamp=2.0, smooth_ms=40.0, adapt_s=1.0, warmup_ms=200.0)
RATE = 24000


def behaviour_input():
    """4 s of -50 dBFS white noise; from 2 s on 0.25 sin(220 Hz) + 0.1 sin(1760 Hz) on top"""
    n = 4 * RATE
    x = np.random.default_rng(0).standard_normal(n) * 10.0 ** (-50.0 / 20.0)
    t = np.arange(n) / RATE
    x[2 * RATE:] += (0.25 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 1760.0 * t))[2 * RATE:]
    return x.astype(np.float32)


def _tone_db(sig, hz):
    t = np.arange(len(sig)) / RATE
    return 20.0 * math.log10(2.0 / len(sig) * abs(np.sum(sig * np.exp(-2j * np.pi * hz * t))))


def behaviour_figures(x, y, delay):
    """(dB by which the output's power over seconds 1 .. 2 lies below the input's, |dB| the 220 Hz and the 1760 Hz tone moved over seconds
    3 .. 4); y is the output for x, `delay` samples late"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    a, b = x[RATE:2 * RATE], y[RATE + delay:2 * RATE + delay]
    down = 10.0 * math.log10(np.mean(a * a) / np.mean(b * b))
    a, b = x[3 * RATE - delay:4 * RATE - delay], y[3 * RATE:4 * RATE]
    return down, abs(_tone_db(b, 220.0) - _tone_db(a, 220.0)), abs(_tone_db(b, 1760.0) - _tone_db(a, 1760.0))


def check_behaviour(x, y, delay):
    down, t220, t1760 = behaviour_figures(x, y, delay)
    print(f"[denoise] behaviour at delay {delay}: noise down {down:.2f} dB, 220 Hz moved {t220:.4f} dB, 1760 Hz moved {t1760:.4f} dB")
    assert down >= 15.0, f"the noise alone comes out only {down:.2f} dB down"
    assert t220 <= 0.1 and t1760 <= 0.1, f"the tones moved by {t220:.3f} / {t1760:.3f} dB"
