"""dpg_bound_records through the C ABI: the per-record keep flags equal the
kept set restated from the oracle's priorities (tests/percentile_ref.py), and
tie to dpg_bound_aggregate on the same inputs: its count, rows and sum per
partition are those of the flagged records, exactly."""
import ctypes

import numpy as np
import pytest
import torch

from tests import percentile_ref as ref

pytestmark = pytest.mark.gpu

SEED, P, T = 0x5EED, 40, 2048
MODE_PER_PID = 1


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, SEED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """~5000 records over 300 privacy ids: id 7 has 3000 records in 2
    partitions (pairs longer than a tile), id 11 has 60 records in 40
    partitions, the rest a few records each.  Shuffled; integer values."""
    rng = np.random.default_rng(17)
    pid = [np.full(3000, 7), np.full(60, 11), rng.integers(100, 398, 1940)]
    pk = [rng.integers(3, 5, 3000), np.arange(60) % P, rng.integers(0, P, 1940)]
    pid, pk = np.concatenate(pid).astype(np.int64), np.concatenate(pk).astype(np.int64)
    o = rng.permutation(len(pid))
    return pid[o], pk[o], rng.integers(-3, 14, len(pid)).astype(np.float64)


def _fields(mode, mpc, mcpp, mask=3, **kw):
    f = dict(mode=mode, sum_mode=1, metric_mask=mask, max_partitions_contributed=mpc,
             max_contributions_per_partition=mcpp, max_contributions=0, min_value=0.0,
             max_value=10.0, min_sum_per_partition=0.0, max_sum_per_partition=0.0,
             n_partitions=P, pid_min=0, pid_count=0, rec_id_offset=0, nonce=99)
    f.update(kw)
    return f


def _run(ctx, pid, pk, val, f, public=None, aggregate=True):
    """keep flags of dpg_bound_records and the partials of dpg_bound_aggregate."""
    from pipelinedp_amd import _native
    n = len(pid)
    d_pid, d_pk = torch.from_numpy(pid).cuda(), torch.from_numpy(pk).cuda()
    d_val = torch.from_numpy(val).cuda()
    bound = _native.fill(_native.BoundParams, f)
    mask = None
    if public is not None:
        from oracle import oracle
        mask = torch.from_numpy(oracle.bitmap(public, P)).cuda()
        bound.public_mask = mask.data_ptr()
    keep = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    part = None
    if aggregate:
        rows, count = (torch.empty(P, dtype=torch.int64, device="cuda") for _ in range(2))
        sums = torch.empty(P, dtype=torch.float64, device="cuda")
        partials = _native.Partials(P, rows.data_ptr(), count.data_ptr(), sums.data_ptr(), None, None)
        ctx.bound_aggregate(d_pid.data_ptr(), d_pk.data_ptr(), d_val.data_ptr(), n, bound,
                            partials, None)
        part = rows, count, sums
    ctx.bound_records(d_pid.data_ptr(), d_pk.data_ptr(), n, bound, keep.data_ptr(), None)
    torch.cuda.synchronize()
    if part is not None:
        part = tuple(t.cpu().numpy() for t in part)
    return keep.cpu().numpy(), part


def _check(ctx, pid, pk, val, f, public=None):
    keep, (rows, count, sums) = _run(ctx, pid, pk, val, f, public)
    n = len(pid)
    want = ref.kept_records(pid, pk, f, SEED, public)
    assert np.array_equal(keep[:n], want)
    if n == 0:
        assert keep[0] == 7  # nothing written
        return
    k = keep[:n].astype(bool)
    assert np.array_equal(count, np.bincount(pk[k], minlength=P))
    pairs = np.unique(np.stack([pid[k], pk[k]]), axis=1)
    assert np.array_equal(rows, np.bincount(pairs[1], minlength=P))
    # integer values: the clipped sums are exact in any order
    assert np.array_equal(sums, np.bincount(pk[k], weights=np.clip(val[k], 0.0, 10.0), minlength=P))


@pytest.mark.parametrize("mcpp", [2, 1])
@pytest.mark.parametrize("n", [None, T - 1, T, T + 1, 0])
def test_cross_and_per_partition(ctx, data, n, mcpp):
    pid, pk, val = (a[:n] for a in data)
    _check(ctx, pid, pk, val, _fields(ref.MODE_CROSS_AND_PER, 3, mcpp))


def test_cross_partition_keeps_every_record_of_a_kept_pair(ctx, data):
    _check(ctx, *data, _fields(ref.MODE_CROSS, 3, 1))


def test_public_mask_and_record_id_offset(ctx, data):
    public = [0, 3, 5, 8, 13, 21, 34, 39]
    _check(ctx, *data, _fields(ref.MODE_CROSS_AND_PER, 3, 2, rec_id_offset=12345), public)
    # record ids that wrap 2^32 inside the call: the low word no longer follows the input order
    _check(ctx, *data, _fields(ref.MODE_CROSS_AND_PER, 3, 2, rec_id_offset=2**32 - 1000), public)


def test_declared_pid_range(ctx, data):
    _check(ctx, *data, _fields(ref.MODE_CROSS_AND_PER, 3, 2, pid_min=7, pid_count=391))


def test_per_privacy_id_is_unsupported(ctx, data):
    from pipelinedp_amd import _native
    f = _fields(MODE_PER_PID, 0, 0, max_contributions=3)
    with pytest.raises(_native.NativeError, match="unsupported"):
        _run(ctx, *data, f, aggregate=False)
