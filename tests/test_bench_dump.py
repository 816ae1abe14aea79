"""bench.py's dump_outputs() (--dump-outputs) on host tensors: whole arrays when they fit, else the same seeded sample of
flat indices for every array of one shape, float32 / float64 only, the whole call under its byte budget.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_small_arrays_are_written_whole(bench, tmp_path):
    s = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    x = torch.linspace(0, 1, 12, dtype=torch.float32).reshape(3, 4)
    got = bench.dump_outputs(str(tmp_path), {"sigma": s, "x_dep": x}, suffix="_rank1")
    assert got == {"sigma": [[3, 4], 12], "x_dep": [[3, 4], 12]}
    a, b = np.load(tmp_path / "sigma_rank1.npy"), np.load(tmp_path / "x_dep_rank1.npy")
    assert a.dtype == np.float64 and np.array_equal(a, s.numpy()) and b.dtype == np.float32 and np.array_equal(b, x.numpy())


def test_large_arrays_are_a_fixed_seeded_sample_within_the_budget(bench, tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"sigma": torch.rand(300, 400, generator=g), "x_dep": torch.rand(300, 400, generator=g),
              "traj_x": [torch.rand(5, 100, generator=g) for _ in range(3)]}          # a list: the members' stack
    budget = 3 * (4096 + 4 * 10000)
    got = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    assert got == {"sigma": [[300, 400], 10000], "x_dep": [[300, 400], 10000], "traj_x": [[3, 5, 100], 1500]}
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["sigma.npy", "traj_x.npy", "x_dep.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(300 * 400, 10000, replace=False))
    for k in ("sigma", "x_dep"):
        v = np.load(tmp_path / "a" / (k + ".npy"))
        assert v.dtype == np.float32 and np.array_equal(v, arrays[k].numpy().reshape(-1)[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "traj_x.npy"), torch.stack(arrays["traj_x"]).numpy())
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)                       # the same sample again
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_a_sample_spread_over_stacked_members(bench, tmp_path):
    parts = [torch.full((50, 60), float(i)) for i in range(4)]
    n = (4096 * 2 + 8000 - 4096) // 4                     # one array: its whole budget less the header allowance
    got = bench.dump_outputs(str(tmp_path), {"sigma": parts}, budget=4096 * 2 + 8000)
    assert got == {"sigma": [[4, 50, 60], n]}
    v = np.load(tmp_path / "sigma.npy")
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(4 * 3000, n, replace=False))
    assert np.array_equal(v, (idx // 3000).astype(np.float32))                         # each element from its own member


def test_integer_outputs_are_refused(bench, tmp_path):
    with pytest.raises((AssertionError, KeyError)):
        bench.dump_outputs(str(tmp_path), {"n": torch.arange(10**6)}, budget=4096 + 1000)
