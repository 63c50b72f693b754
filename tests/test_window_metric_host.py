"""The windowed error measure of tests/helpers.py (window_errors): what the per-window gate of test_gpu_tile_edges.py sees and the
whole-tensor relative rms cannot."""
import torch

from helpers import rel_rms, window_errors, window_starts


def test_a_two_column_error_passes_the_whole_tensor_gate_and_trips_the_window_gate():
    """A block output of the 96-channel level at T = 129 (3096 columns) whose last two columns are off by 1e-4 of the tensor's rms: the
    whole-tensor figure is 1e-4 sqrt(2 / 3096) = 2.5e-6, below the 3e-6 block gate; the window that ends on the last column shows
    1e-4 sqrt(2 / 32) = 2.5e-5."""
    g = torch.Generator().manual_seed(0)
    truth = torch.randn(1, 96, 3096, generator=g, dtype=torch.float64)
    x = truth.clone()
    x[..., -2:] += 1e-4 * float(truth.pow(2).mean().sqrt())
    assert rel_rms(x, truth) < 3e-6
    e = window_errors(x, truth)
    assert e.shape == (1, len(window_starts(3096)))
    assert float(e.max()) > 2e-5
    assert int(e[0].argmax()) == e.shape[1] - 1, "the worst window is the one aligned to the last column"
    assert float(e[0, :-2].max()) == 0.0, "windows that do not hold the last two columns see nothing"
    assert float(window_errors(truth, truth).max()) == 0.0


def test_windows_cover_every_column_and_the_last_one_ends_on_the_last_column():
    for n in (33, 47, 48, 64, 250, 3096):
        st = window_starts(n)
        assert st[0] == 0 and st[-1] == n - 32 and st == sorted(set(st))
        assert all(b - a <= 16 for a, b in zip(st, st[1:])), "stride width // 2: no column between two windows"


def test_short_rows_are_one_window():
    g = torch.Generator().manual_seed(1)
    for n in (1, 6, 31, 32):
        truth = torch.randn(2, 5, n, generator=g, dtype=torch.float64)
        x = truth + 1e-3
        e = window_errors(x, truth)
        assert e.shape == (2, 1) and window_starts(n) == [0]
        for b in range(2):      # one window over the whole row = the row's relative rms
            assert abs(float(e[b, 0]) - rel_rms(x[b], truth[b])) <= 1e-12 * rel_rms(x[b], truth[b])
    assert window_errors(torch.zeros(1, 2, 33), torch.ones(1, 2, 33, dtype=torch.float64)).shape == (1, 2)


def test_the_error_is_relative_to_the_rows_own_rms():
    truth = torch.ones(2, 3, 100, dtype=torch.float64)
    truth[1] *= 1e3
    x = truth.clone()
    x[:, :, 40:72] += 0.5          # windows start every 16 columns: [32, 64) and [48, 80) hold 24 of the 32 columns, none holds all
    e = window_errors(x, truth)
    assert abs(float(e[0].max()) - 0.5 * (24 / 32) ** 0.5) < 1e-12
    assert abs(float(e[1].max()) - 0.5e-3 * (24 / 32) ** 0.5) < 1e-12
