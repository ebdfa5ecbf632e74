"""Tails of the level-1 scatter's software pipeline: k_scatter loads the
next sub-tile (SUB = 8 x 1024 records in piece mode) while the current one
is scanned, staged and written, clamped into the sub-tile, and after the
last sub-tile of a tile it loads the first one of the workgroup's next tile.
The sizes below are those at which that prefetch can go wrong: no successor
tile, a one-record tail (no 16-byte pair inside the tile: loaded singly, or
in piece mode as the pair that starts one record before it), an odd tail
(the pair clamp), and tile counts that are / are not a multiple of the
workgroup count.  N0 = 2^22 is the smallest input that takes the
histogram-free level 1.

Every case compares the partials with the oracle (privacy-id counts and
counts bit-exact, sums to 1e-9) and asserts the path its stage times name,
so a silent redo through the histogram fallback does not pass."""
import numpy as np
import pytest
import torch

import bench
import pipelinedp_amd as pdp
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x71A115
SUB = 8 * 1024
N0 = 1 << 22
NMAX = N0 + 256 * SUB
P = 100_000
U = 50_000  # ~84 (N0) to ~126 (NMAX) records per privacy id


def _params(mpc=8, mcpp=2):
    return pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=mpc,
        max_contributions_per_partition=mcpp, min_value=0.0, max_value=10.0)


def _run_and_check(pid, pk, val, P, pid_range):
    backend = pdp.MI355XBackend(device=0, seed=SEED)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    cols = pdp.ColumnarData(pid=torch.from_numpy(pid).cuda(), pk=torch.from_numpy(pk).cuda(),
                            value=torch.from_numpy(val).cuda(), n_partitions=P,
                            privacy_id_range=pid_range)
    res = pdp.DPEngine(acc, backend).aggregate(cols, _params(), pdp.DataExtractors("pid", "pk", "value"))
    acc.compute_budgets()
    res.noise_enabled = False
    res.nonce = 77
    res.materialize()
    got = {k: v.cpu().numpy() for k, v in res.last_partials.items() if v is not None}
    ref = oracle.bound_aggregate(pid, pk, val, res.last_bound_fields, SEED)
    assert np.array_equal(got["rows"], ref["rows"])
    assert np.array_equal(got["count"], ref["count"])
    assert np.allclose(got["sum"], ref["sum"], rtol=1e-9, atol=1e-9)
    return backend.ctx.stage_times()


@pytest.fixture(scope="module")
def data():
    """The bench generator at the largest size; every case takes a prefix
    (privacy ids and partitions are drawn independently per record)."""
    pid, pk, val = bench.host_sample(NMAX, U, P, 808)
    return pid.astype(np.int64), pk.astype(np.int64), val


def _prefix(data, n):
    pid, pk, val = data
    return pid[:n], pk[:n], val[:n]


@pytest.mark.parametrize("extra", [0, 1, SUB - 1, 255 * SUB + 2, 256 * SUB],
                         ids=["full", "one", "odd", "255sub+2", "256sub"])
def test_piece_mode_tails(built, data, monkeypatch, extra):
    """The histogram-free level 1 at N0 + extra records."""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    pid, pk, val = _prefix(data, N0 + extra)
    st = _run_and_check(pid, pk, val, P, (0, U))
    assert "partition1:pieces" in st and "partition2:team" in st
    assert "partition1:hist" not in st


@pytest.mark.parametrize("extra", [1, SUB - 1], ids=["one", "odd"])
def test_histogram_level1_tails(built, data, monkeypatch, extra):
    """The histogram level 1 (DPG_L1_PIECES=0): tiles of several sub-tiles
    and the change from one tile to the next."""
    monkeypatch.setenv("DPG_L1_PIECES", "0")
    pid, pk, val = _prefix(data, N0 + extra)
    st = _run_and_check(pid, pk, val, P, (0, U))
    assert "partition1:hist" in st and "partition1:pieces" not in st


def test_twelve_byte_records_tail(built):
    """P = 1e8 uniform partitions and 2^23 privacy ids: 65 key + index bits,
    so 12-byte records and the grouped level 1."""
    n, P12, U12 = N0 + SUB - 1, 100_000_000, 1 << 23
    rng = np.random.default_rng(1212)
    pid = rng.integers(0, U12, n).astype(np.int64)
    pk = rng.integers(0, P12, n).astype(np.int64)
    val = rng.uniform(-1.0, 11.0, n)
    st = _run_and_check(pid, pk, val, P12, (0, U12))
    assert "partition1:scatter" in st
    assert "partition1:pieces" not in st


def test_piece_mode_one_record_tail_range_error(built, data, monkeypatch):
    """The one-record tail tile's privacy id is past the declared range (high
    word differs, low word in range): the tail's load keeps the whole id,
    and the call fails with the key-range error."""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    pid, pk, val = _prefix(data, N0 + 1)
    bad = pid.copy()
    bad[-1] += 1 << 32
    with pytest.raises(Exception, match="range"):
        _run_and_check(bad, pk, val, P, (0, U))
