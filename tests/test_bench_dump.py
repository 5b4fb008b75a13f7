"""bench.py --dump-outputs: the last timed step's recorded rows as <name>.npy, a fixed sample of the
chains when the records are larger than the limit; and a plain run (no --full) measures the headline
alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _records(C):
    import torch
    g = torch.Generator().manual_seed(3)
    return {"x": torch.randn(7, C, 30, dtype=torch.float64, generator=g),
            "b": torch.randn(7, C, 76, dtype=torch.float64, generator=g)}


def test_dump_writes_every_chain_under_the_limit(tmp_path):
    import bench
    recs = _records(33)
    bench.dump_outputs(str(tmp_path / "d"), recs)
    assert sorted(os.listdir(tmp_path / "d")) == ["b.npy", "x.npy"]
    for name, t in recs.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float64
        assert np.array_equal(a, t.numpy())


def test_dump_samples_the_same_chains_every_time(tmp_path, monkeypatch):
    import bench
    C = 33
    recs = _records(C)
    per_chain = 7 * (30 + 76) * 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * per_chain + 5)
    bench.dump_outputs(str(tmp_path / "a"), recs)
    bench.dump_outputs(str(tmp_path / "b"), recs)
    xa, ba = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "b.npy")
    assert xa.shape == (7, 10, 30) and ba.shape == (7, 10, 76)
    assert xa.nbytes + ba.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(xa, np.load(tmp_path / "b" / "x.npy"))
    assert np.array_equal(ba, np.load(tmp_path / "b" / "b.npy"))
    # the kept rows are whole chains of the record, the same ones in x and b, in increasing order
    x, b = recs["x"].numpy(), recs["b"].numpy()
    idx = [int(np.flatnonzero((x[0] == row).all(axis=1))[0]) for row in xa[0]]
    assert idx == sorted(set(idx))
    assert np.array_equal(xa, x[:, idx]) and np.array_equal(ba, b[:, idx])
    # two ranks share the limit
    bench.dump_outputs(str(tmp_path / "c"), recs, rank=1, world=2)
    assert np.load(tmp_path / "c" / "x_rank1.npy").shape == (7, 5, 30)


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_dumps_its_last_step(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--chains", "128", "--sweeps-per-launch", "10", "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "chain-iters/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - 128 * 10 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["secondary"] == {} and line["cpu_baseline"] is None and line["ess_per_s"] is None
    x, b = np.load(tmp_path / "d" / "x.npy"), np.load(tmp_path / "d" / "b.npy")
    assert x.dtype == b.dtype == np.float64
    assert x.shape == (10, 128, 30) and b.shape[:2] == (10, 128)
    assert np.isfinite(x).all() and np.isfinite(b).all()
    assert (x >= -9).all() and (x <= -4).all()        # log10 rho / 2 inside the prior [1e-18, 1e-8]
