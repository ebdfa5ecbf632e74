"""dpg_shard_records_wide / dpg_check_shard_wide through the C ABI, one process:
the split equals its numpy restatement exactly (dest = distributed.
shard_of_wide(pid), a stable argsort of dest, a bincount), at the sizes where
the tiling changes path, with and without a value column, over ids that include
the extremes of int64 and ids that differ only in their high 32 bits -- which
distributed.shard_of sends to one rank and shard_of_wide does not."""
import numpy as np
import pytest
import torch

RANKS = (1, 2, 3, 7, 8, 64)
SIZES = (0, 1, 2047, 2048, 2049, 10_007)
I64 = np.iinfo(np.int64)
EDGE = np.array([0, -1, 2**32 - 1, 2**32, I64.max, I64.min], dtype=np.int64)
N_HIGH = 2000  # ids user << 32: the low words are all zero


def _records():
    n = max(SIZES)
    rng = np.random.default_rng(23)
    pid = rng.integers(-2**62, 2**62, n).astype(np.int64)
    pid[:len(EDGE)] = EDGE
    pid[-len(EDGE):] = EDGE
    pid[100:100 + N_HIGH] = np.arange(1, N_HIGH + 1, dtype=np.int64) << 32
    pk = rng.integers(0, 1 << 40, n).astype(np.int64)
    val = rng.uniform(-1.0, 11.0, n)
    return pid, pk, val


def _dest(pid, world):
    from pipelinedp_amd import distributed
    return distributed.shard_of_wide(torch.from_numpy(pid), world).numpy()


@pytest.mark.parametrize("world", [w for w in RANKS if w > 1])
def test_high_word_ids_spread_only_under_the_wide_function(world):
    """Runs without a GPU: the ids this module feeds the kernels show the
    difference between the two shard functions."""
    from pipelinedp_amd import distributed
    high = torch.from_numpy(_records()[0][100:100 + N_HIGH])
    assert len(torch.unique(distributed.shard_of(high, world))) == 1
    wide = distributed.shard_of_wide(high, world)
    counts = torch.bincount(wide, minlength=world)
    assert int(wide.min()) >= 0 and int(wide.max()) < world
    # every rank gets some, none more than three times its share
    assert (counts > 0).all() and int(counts.max()) <= 3 * N_HIGH // world + 8


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    return _records()


def _split(ctx, pid, pk, val, world):
    n = len(pid)
    d_pid, d_pk = torch.from_numpy(pid).cuda(), torch.from_numpy(pk).cuda()
    d_val = torch.from_numpy(val).cuda() if val is not None else None
    # sentinels: entries the split must overwrite (or, for n = 0, leave alone)
    o_pid = torch.full((n + 4,), -7, dtype=torch.int64, device="cuda")
    o_pk = torch.full((n + 4,), -7, dtype=torch.int64, device="cuda")
    o_val = torch.full((n + 4,), -7.0, dtype=torch.float64, device="cuda") \
        if val is not None else None
    counts = torch.full((world,), -7, dtype=torch.int64, device="cuda")
    ctx.shard_records_wide(d_pid.data_ptr(), d_pk.data_ptr(),
                           d_val.data_ptr() if d_val is not None else None, n, world,
                           o_pid.data_ptr(), o_pk.data_ptr(),
                           o_val.data_ptr() if o_val is not None else None, counts.data_ptr(),
                           None)
    torch.cuda.synchronize()
    for o in (o_pid, o_pk) + ((o_val,) if o_val is not None else ()):
        assert (o[n:] == -7).all()  # nothing is written past the records
    return (o_pid[:n].cpu().numpy(), o_pk[:n].cpu().numpy(),
            o_val[:n].cpu().numpy() if o_val is not None else None, counts.cpu().numpy())


def _check_split(ctx, pid, pk, val, world):
    dest = _dest(pid, world)
    order = np.argsort(dest, kind="stable")
    g_pid, g_pk, g_val, g_counts = _split(ctx, pid, pk, val, world)
    assert np.array_equal(g_counts, np.bincount(dest, minlength=world))
    assert np.array_equal(g_pid, pid[order])
    assert np.array_equal(g_pk, pk[order])
    if val is not None:
        assert np.array_equal(g_val, val[order])
    return order


@pytest.mark.gpu
@pytest.mark.parametrize("world", RANKS)
def test_split_equals_numpy(ctx, records, world):
    pid, pk, val = records
    for n in SIZES:
        order = _check_split(ctx, pid[:n], pk[:n], val[:n], world)
        if world == 1:  # an identity copy
            assert np.array_equal(order, np.arange(n))


@pytest.mark.gpu
@pytest.mark.parametrize("world", RANKS)
def test_split_without_values(ctx, records, world):
    pid, pk, _ = records
    for n in (1, 2049, max(SIZES)):
        _check_split(ctx, pid[:n], pk[:n], None, world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", RANKS)
def test_check_shard_wide(ctx, records, world):
    pid = records[0]
    d_pid = torch.from_numpy(pid).cuda()
    n_bad = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    dest = _dest(pid, world)
    for rank in sorted({0, world // 2, world - 1}):
        for n in SIZES:
            ctx.check_shard_wide(d_pid.data_ptr(), n, world, rank, n_bad.data_ptr(), None)
            assert int(n_bad.item()) == int((dest[:n] != rank).sum())
        # a correctly sharded slice: nothing to report
        mine = torch.from_numpy(pid[dest == rank]).cuda()
        ctx.check_shard_wide(mine.data_ptr(), mine.numel(), world, rank, n_bad.data_ptr(), None)
        assert int(n_bad.item()) == 0


@pytest.mark.gpu
def test_the_narrow_calls_still_split_by_shard_of(ctx, records):
    """The two functions are two instantiations of one kernel: the existing
    entry points keep the low-32-bit owner."""
    from pipelinedp_amd import distributed
    pid, pk, _ = records
    world = 8
    dest = distributed.shard_of(torch.from_numpy(pid), world).numpy()
    d_pid, d_pk = torch.from_numpy(pid).cuda(), torch.from_numpy(pk).cuda()
    o_pid, o_pk = torch.empty_like(d_pid), torch.empty_like(d_pk)
    counts = torch.empty(world, dtype=torch.int64, device="cuda")
    ctx.shard_records(d_pid.data_ptr(), d_pk.data_ptr(), None, len(pid), world, o_pid.data_ptr(),
                      o_pk.data_ptr(), None, counts.data_ptr(), None)
    assert np.array_equal(o_pid.cpu().numpy(), pid[np.argsort(dest, kind="stable")])
    assert np.array_equal(counts.cpu().numpy(), np.bincount(dest, minlength=world))
    assert not np.array_equal(dest, _dest(pid, world))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [0, 65])
def test_rank_count_out_of_range_raises(ctx, world):
    from pipelinedp_amd import _native
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    counts = torch.zeros(65, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.shard_records_wide(x.data_ptr(), x.data_ptr(), None, 64, world, x.data_ptr(),
                               x.data_ptr(), None, counts.data_ptr(), None)
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.check_shard_wide(x.data_ptr(), 64, world, 0, counts.data_ptr(), None)


@pytest.mark.gpu
def test_two_to_the_31_records_are_unsupported(ctx):
    from pipelinedp_amd import _native
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError, match="unsupported"):
        ctx.shard_records_wide(x.data_ptr(), x.data_ptr(), None, 1 << 31, 2, x.data_ptr(),
                               x.data_ptr(), None, x.data_ptr(), None)
