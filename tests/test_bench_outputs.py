"""bench.py's `--dump-outputs DIR` (what the last timed step left, float32, capped at 64 MB by a seeded row sample) and the
plain line (no CPU legs, no parity block without `--full`).  The writer is checked on CPU with a stand-in planner; one
tiny end-to-end run of each form on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


class _Engine(object):
    def __init__(self, b, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.traj = torch.rand(b, n, 3, generator=g)
        self.lam = torch.rand(b, n + 1, generator=g)
        self.cm = torch.rand(b, n, generator=g)


class _Onf(object):
    flat_parameters = torch.arange(10, dtype=torch.float32)


class _Planner(object):
    def __init__(self, b, n, seed=0):
        self.engine, self.onf = _Engine(b, n, seed), _Onf()

    def get_paths(self):
        t = self.engine.traj
        return torch.cat([t[:, :1], t, t[:, -1:]], 1).numpy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_what_the_planner_holds(tmp_path):
    p = _Planner(6, 5)
    bench.dump_outputs(str(tmp_path / "frozen"), p, False, 1, 0)
    got = _load(str(tmp_path / "frozen"))
    assert sorted(got) == ["cm", "lam", "paths"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["paths"], p.get_paths()) and got["paths"].shape == (6, 7, 3)
    assert np.array_equal(got["lam"], p.engine.lam.numpy()) and np.array_equal(got["cm"], p.engine.cm.numpy())
    bench.dump_outputs(str(tmp_path / "learn"), p, True, 1, 0)
    assert np.array_equal(_load(str(tmp_path / "learn"))["onf_params"], np.arange(10, dtype=np.float32))
    bench.dump_outputs(str(tmp_path / "rank1"), p, False, 1, 1)          # only rank 0 writes
    assert not os.path.exists(str(tmp_path / "rank1"))


def test_dump_above_the_limit_keeps_the_same_seeded_rows(tmp_path, monkeypatch):
    p = _Planner(40, 5)
    per_row = (7 * 3 + 6 + 5) * 4
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * per_row + 3)
    bench.dump_outputs(str(tmp_path / "a"), p, False, 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), _Planner(40, 5), False, 1, 0)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(x.nbytes for x in a.values()) <= 10 * per_row + 3
    assert a["paths"].shape == (10, 7, 3) and a["lam"].shape == (10, 6) and a["cm"].shape == (10, 5)
    rows = [int(np.flatnonzero((p.get_paths() == r).all((1, 2)))[0]) for r in a["paths"]]
    assert rows == sorted(rows) and len(set(rows)) == 10                  # sorted sample without repeats...
    assert np.array_equal(a["lam"], p.engine.lam.numpy()[rows])           # ...the same rows in every file
    assert np.array_equal(a["cm"], p.engine.cm.numpy()[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)                     # fixed seed: the same sample every run


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_and_full_runs_on_the_gpu(tmp_path):
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch-per-gpu", "64", "--fit-iters", "2", "--spin-up", "0"]
    lines, dumps = [], []
    for k, extra in enumerate((["--dump-outputs", str(tmp_path / "a")], ["--dump-outputs", str(tmp_path / "b")],
                               ["--full", "--cpu-seconds", "0.2"])):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + extra, capture_output=True,
                             text=True, timeout=280)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [l for l in res.stdout.splitlines() if l.strip()]
        assert len(out) == 1, res.stdout
        lines.append(json.loads(out[0]))
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["metric"] == "waypoint-evals/sec" and d["unit"] == "waypoint-evals/s" and d["dtype"] == "f32"
    assert "parity" not in lines[0] and "cpu_baseline" not in lines[0]    # a plain run stops at the line
    assert lines[2]["parity"]["ok"] and lines[2]["cpu_baseline"]["value"] > 0
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["cm", "lam", "paths"]
    assert a["paths"].shape == (64, 258, 3) and a["lam"].shape == (64, 257) and a["cm"].shape == (64, 256)
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)                     # same arguments, same inputs, same outputs
