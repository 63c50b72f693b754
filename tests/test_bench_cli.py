"""bench.py's launch contract: `python bench.py --gpus N` launches its own N ranks (the driver calls it both ways), the N > 1
branch (RCCL communicator, gather into rank 0's landing buffer, its JSON keys) is rehearsed at world size 1 on a real GPU, and
every line carries the parity block."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_gpus_2_without_a_launcher_spawns_two_ranks_and_fails_clearly_without_gpus():
    """On a box with fewer than 2 GPUs the self-launched ranks must stop with a message that says what is missing
    (not a SystemExit telling the caller to use another launcher, not a hang)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("box has 2+ GPUs: the launch would succeed")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], 300)
    assert r.returncode != 0
    err = r.stdout + r.stderr
    assert "GPU(s)" in err and "one process per GPU" in err, err[-2000:]


@pytest.mark.gpu
def test_force_dist_rehearses_the_multi_gpu_branch_at_world_size_1():
    r = _run(["--force-dist", "--steps", "3", "--warmup", "1"], 900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 1 and j["rccl_ranks"] == 1 and j["forced_dist_rehearsal"] is True
    assert "configs[3]" in j["config"]["workload"] and j["config"]["index_vectors"] == 100000
    assert j["gather_ms"] is not None and j["gather_ms"] > 0 and j["gather_bytes_per_rank"] == 64 * 96000 * 4
    assert j["n1_same_workload_value"] > 0 and 0.5 < j["scaling_efficiency"] <= 1.25      # (two 3-step timings of the same work at world size 1: a sanity range, not a measurement)
    assert j["value"] > 3.2e6                       # north_star's 200x real time, by a wide margin
    p = j["parity"]
    assert p["knn_idx_equal"] and p["rms_vs_golden_max"] <= 1e-4 and p["ok"], p


@pytest.mark.gpu
def test_default_line_carries_parity_roofline_and_cpu_baseline_keys():
    r = _run(["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-stream"], 900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 1 and "configs[1]" in j["config"]["workload"] and j["dtype"].startswith("f32")
    p = j["parity"]
    assert "timed" in p["checked"] and len(p["rms_vs_golden"]) == 4
    assert p["knn_idx_equal"] and p["knn_idx_mismatches"] == 0 and p["rms_vs_golden_max"] <= 1e-4 and p["ok"], p
    assert p["drawn_equals_injected_hash"] is True, "the timed instantiation (phases drawn in-kernel) must equal the injected restatement of its hash"
    rf = j["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and 0 < rf["frac"] < 1 and rf["launch_ms"] > 0


def test_dump_outputs_keeps_a_seeded_sample_under_the_cap(tmp_path, monkeypatch):
    """Above the size cap every array keeps a fixed sample of its rows, the same on every call, and the files stay under the cap."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 1 << 20)
    x = torch.randn(4, 64, 2000)
    info = bench.dump_outputs(str(tmp_path / "a"), {"wave_gathered": x})
    bench.dump_outputs(str(tmp_path / "b"), {"wave_gathered": x})
    assert info["wave_gathered"]["shape"] == [4, 64, 2000] and 0 < info["wave_gathered"]["rows_kept"] < 256
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 1 << 20
    w, rows = np.load(tmp_path / "a" / "wave_gathered.npy"), np.load(tmp_path / "a" / "wave_gathered_rows.npy")
    assert w.dtype == np.float32 and rows.dtype == np.float64
    assert np.array_equal(w, x.reshape(-1, 2000)[torch.from_numpy(rows.astype(np.int64))].numpy())
    assert np.array_equal(w, np.load(tmp_path / "b" / "wave_gathered.npy"))
    # below the cap the array is written whole
    small = bench.dump_outputs(str(tmp_path / "c"), {"wave": x[0]})
    assert small["wave"]["rows_kept"] is None and np.array_equal(np.load(tmp_path / "c" / "wave.npy"), x[0].numpy())


@pytest.mark.gpu
def test_dump_outputs_repeats_from_run_to_run(tmp_path):
    """--dump-outputs: the last timed step's waveforms, float32, the same in two runs with the same arguments (inputs and the
    noise phases the library draws are seeded), and --steps is the number of timed steps the line reports."""
    import numpy as np
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        r = _run(["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-stream", "--no-parity", "--dump-outputs", str(d)], 900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        j = _line(r.stdout)
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["dump_outputs"]["arrays"]["wave"]["shape"] == [64, 96000]
        w = np.load(d / "wave.npy")
        assert w.dtype == np.float32 and w.shape == (64, 96000) and np.isfinite(w).all() and np.abs(w).max() > 0
        outs.append(w)
    assert np.array_equal(outs[0], outs[1])
