"""bench.py --dump-outputs: what is written, how much, and that the same arguments give the same files.  The helpers run on host
tensors here; on the GPU the same code samples the device slab (tests/test_gpu_bench_contract.py)."""
import os

import numpy as np
import pytest
import torch

import bench
from phyloligo_amd.dist import RowBlockPlan


def _dump(tmp, plan, n):
    """every rank's slab entry holds its own position in the n x n matrix, so a sample says where it came from"""
    for rank in range(plan.world):
        slab, mirrors = plan.allocate(rank, "cpu", torch.float64)
        lo, hi = plan.rows(rank)
        slab.copy_(torch.arange(lo, hi, dtype=torch.float64)[:, None] * n + torch.arange(n, dtype=torch.float64))
        for m in mirrors:
            if m is not None:
                m.fill_(-1.0)
        bench.dump_outputs(str(tmp), plan, rank, slab, mirrors)
    return sorted(os.listdir(tmp))


def test_small_matrix_is_written_whole(tmp_path):
    n = 300
    assert _dump(tmp_path, RowBlockPlan(n, 1), n) == ["distances_all.npy"]
    a = np.load(tmp_path / "distances_all.npy")
    assert a.dtype == np.float64 and np.array_equal(a, np.arange(n * n, dtype=np.float64).reshape(n, n))


@pytest.mark.parametrize("world", [1, 3])
def test_large_matrix_is_a_seeded_sample_within_the_budget(tmp_path, monkeypatch, world):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    n = 1000
    names = _dump(tmp_path / "a", RowBlockPlan(n, world), n)
    assert names == _dump(tmp_path / "b", RowBlockPlan(n, world), n)
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
        total += a.nbytes
        if f.endswith("_rows.npy") and "mirror" not in f:          # whole rows of the matrix, in order, none twice
            assert a.shape[1] >= 1 and np.all(np.diff(a[:, 0]) > 0)
            assert np.array_equal(a - a[:, :1], np.broadcast_to(np.arange(a.shape[1], dtype=np.float64), a.shape))
    assert total <= 1 << 20
    if world == 1:
        assert names == ["distances_entries.npy", "distances_rows.npy"]
        e = np.load(tmp_path / "a" / "distances_entries.npy")
        assert e.size == (1 << 19) // 8 and e.min() >= 0 and e.max() < n * n and len(np.unique(e)) > e.size // 2
    else:
        assert all(f.startswith("distances_rank") for f in names)
        assert {f.split("_")[1] for f in names} == {"rank%d" % r for r in range(world)}
