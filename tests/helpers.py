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
