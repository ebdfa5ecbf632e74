"""Host-side logic of bench.py (no GPU): the PMC traffic of
profiles/hbm_traffic*.json is attached only to the workload its passes
measured (configs[1] / configs[3] private at their default sizes), never
to an envelope input or the public-partition line; --dump-outputs writes
float64 arrays, whole or as the same seeded row sample every time."""
import argparse
import os

import numpy as np
import torch

import bench


def _args(**kw):
    a = dict(records=1_000_000_000, pids=10_000_000, partitions=1_000_000, mpc=8, mcpp=2,
             public=False, pid_cap=1000.0)
    a.update(kw)
    return argparse.Namespace(**a)


def test_default_workloads_carry_traffic():
    assert bench._default_workload(_args(), c4=False)
    assert bench._default_workload(_args(partitions=100_000_000, mpc=50, mcpp=4), c4=True)


def test_envelope_and_public_lines_do_not():
    assert not bench._default_workload(_args(pids=1_000_000), c4=False)
    assert not bench._default_workload(_args(records=2_000_000_000, pids=20_000_000), c4=False)
    assert not bench._default_workload(
        _args(partitions=100_000_000, mpc=50, mcpp=4, public=True), c4=True)
    tj, why = bench._traffic(False, 1_000_000_000, default=False)
    assert tj is None and "default" in why


def test_dump_writes_float64_arrays_whole(tmp_path):
    ids = torch.arange(1000, dtype=torch.int64)
    vals = torch.arange(3000, dtype=torch.float64).reshape(1000, 3) * 0.5
    bench._dump(str(tmp_path), {"partition_ids": ids, "values": vals})
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert list(got) == ["partition_ids.npy", "values.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["partition_ids.npy"], ids.numpy())
    assert np.array_equal(got["values.npy"], vals.numpy())


def test_dump_samples_a_large_output_the_same_way_every_time(tmp_path):
    # 4 columns of 8 bytes per row + the row index: above DUMP_BYTES at n rows
    n = bench.DUMP_BYTES // 40 + 1000
    ids = torch.arange(n, dtype=torch.int64) * 3
    vals = (torch.arange(n, dtype=torch.float64)[:, None] + torch.tensor([0.0, 0.25, 0.5]))
    for d in ("a", "b"):
        bench._dump(str(tmp_path / d), {"partition_ids": ids, "values": vals}, "_rank1")
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["partition_ids_rank1.npy", "rows_rank1.npy", "values_rank1.npy"]
    assert all(np.array_equal(a[f], b[f]) and a[f].dtype == np.float64 for f in a)
    rows = a["rows_rank1.npy"].astype(np.int64)
    assert len(rows) == bench.DUMP_BYTES // 40 and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(a["partition_ids_rank1.npy"], rows * 3.0)
    assert np.array_equal(a["values_rank1.npy"][:, 2], rows + 0.5)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES
