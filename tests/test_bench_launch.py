"""bench.py's launch path and window bookkeeping on CPU (no GPU).

* ``--gpus 2`` starts two ranks itself (torch.distributed.run child, gloo in
  the --dry-run rehearsal) and rank 0 prints one JSON line with n_gpus 2;
* the timed window is exactly --steps steps (F-step launches, remainder
  last), so the line's ``steps``/``warmup`` equal the flags;
* the Python/NumPy CPU baseline runs P processes x 1 env.
"""
import json
import subprocess
import sys

import pytest

from helpers import REPO

sys.path.insert(0, str(REPO))
import bench  # noqa: E402


def test_launch_sizes_cover_exactly():
    assert bench.launches(20, 16) == [16, 4]
    assert bench.launches(5, 16) == [5]
    assert bench.launches(5408, 16) == [16] * 338
    assert bench.launches(0, 16) == []
    for k in (1, 15, 16, 17, 100, 5408):
        assert sum(bench.launches(k, 16)) == k


def test_gpus2_launches_two_ranks_dry_run():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--dry-run"], cwd=str(REPO),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks"] == [0, 1] and rec["dry_run"] is True


def test_world_size_mismatch_is_rejected():
    env = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}
    import os
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--dry-run"], cwd=str(REPO),
                       capture_output=True, text=True, timeout=120, env={**os.environ, **env})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_plain_run_is_the_headline_alone_and_full_keeps_the_legs():
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.steps == 20 and plain.warmup == 5
    assert (plain.episode_window, plain.fuse_check, plain.single_step_check, plain.simple) == (0, 0, 0, 0)
    assert plain.room_sets == "none" and plain.collector == "none" and plain.cpu_seconds == 0
    full = bench.parse(["--full", "--simple", "0"])
    assert full.full and full.simple == 0 and full.episode_window == 1 and full.fuse_check == 16
    assert full.collector == "lstm,mlp" and full.room_sets == "P2_training,P3_training" and full.cpu_seconds == 8.0


def test_dump_outputs_writes_the_last_step_as_float32(tmp_path, monkeypatch):
    np = pytest.importorskip("numpy")
    torch = pytest.importorskip("torch")
    from voxnav.env import Rollout
    F, N = 3, 10
    g = torch.Generator().manual_seed(0)
    out = Rollout(torch.randn(F, N, 80, generator=g), torch.randn(F, N, generator=g),
                  torch.randint(0, 2, (F, N), generator=g, dtype=torch.uint8),
                  torch.randint(0, 2, (F, N), generator=g, dtype=torch.uint8), None)
    bench.dump_outputs(tmp_path / "a", out, 2, 0, 1)       # the last launch ran 2 steps: row 1
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert sorted(got) == ["obs", "reward", "terminated", "truncated"]
    for k, a in got.items():
        assert a.dtype == np.float32
        assert (a == getattr(out, k)[1].float().numpy()).all()
    # over the byte budget: the same seeded sample of agents in every run, within the budget
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096 + 4 * 83 * 4)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, out, 3, 1, 2)
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert sorted(b) == ["obs_rank1", "reward_rank1", "terminated_rank1", "truncated_rank1"]
    assert b["obs_rank1"].shape == (4, 80) and b["reward_rank1"].shape == (4,)
    assert sum(a.nbytes for a in b.values()) <= 4 * 83 * 4
    rows = [i for i in range(N) if any((out.obs[2, i].numpy() == r).all() for r in b["obs_rank1"])]
    assert len(rows) == 4 and (b["reward_rank1"] == out.reward[2, rows].numpy()).all()
    for p in (tmp_path / "b").glob("*.npy"):
        assert (np.load(tmp_path / "c" / p.name) == b[p.stem]).all()


def test_python_numpy_baseline_runs_processes():
    v, steps, _ = bench.python_numpy_baseline("8x8x4", 4, 1.0, 2)
    assert steps >= 512 and v > 0
