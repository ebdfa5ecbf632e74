"""dpg_shard_records / dpg_check_shard through the C ABI, one process: the
split equals its numpy restatement exactly (dest = shard(pid), a stable
argsort of dest, a bincount), at the sizes where the tiling changes path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 8, 64)
I64 = np.iinfo(np.int64)
EDGE = np.array([0, -1, 2**32 - 1, 2**32, I64.min, I64.max], dtype=np.int64)


def _shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (pid.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


def _sizes():
    from pipelinedp_amd import _native
    T = _native.SHARD_TILE
    return (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7)


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    """One host dataset of the largest size; every case takes a prefix.  The
    edge ids sit at the front (so that short prefixes have them) and at the
    end of the longest prefix."""
    n = max(_sizes())
    rng = np.random.default_rng(21)
    pid = rng.integers(-2**40, 2**40, n).astype(np.int64)
    pid[:len(EDGE)] = EDGE
    pid[-len(EDGE):] = EDGE
    pk = rng.integers(0, 1 << 40, n).astype(np.int64)
    val = rng.uniform(-1.0, 11.0, n)
    return pid, pk, val


def _split(ctx, pid, pk, val, world):
    n = len(pid)
    d_pid, d_pk = torch.from_numpy(pid).cuda(), torch.from_numpy(pk).cuda()
    d_val = torch.from_numpy(val).cuda() if val is not None else None
    # sentinels: entries the split must overwrite (or, for n = 0, leave alone)
    o_pid = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    o_pk = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    o_val = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device="cuda") \
        if val is not None else None
    counts = torch.full((world,), -7, dtype=torch.int64, device="cuda")
    ctx.shard_records(d_pid.data_ptr(), d_pk.data_ptr(),
                      d_val.data_ptr() if d_val is not None else None, n, world,
                      o_pid.data_ptr(), o_pk.data_ptr(),
                      o_val.data_ptr() if o_val is not None else None, counts.data_ptr(), None)
    torch.cuda.synchronize()
    return (o_pid[:n].cpu().numpy(), o_pk[:n].cpu().numpy(),
            o_val[:n].cpu().numpy() if o_val is not None else None, counts.cpu().numpy())


def _check_split(ctx, pid, pk, val, world):
    dest = _shard_np(pid, world)
    order = np.argsort(dest, kind="stable")
    g_pid, g_pk, g_val, g_counts = _split(ctx, pid, pk, val, world)
    assert np.array_equal(g_counts, np.bincount(dest, minlength=world))
    assert np.array_equal(g_pid, pid[order])
    assert np.array_equal(g_pk, pk[order])
    if val is not None:
        assert np.array_equal(g_val, val[order])
    return order


@pytest.mark.parametrize("world", RANKS)
def test_split_equals_numpy(ctx, records, world):
    pid, pk, val = records
    for n in _sizes():
        order = _check_split(ctx, pid[:n], pk[:n], val[:n], world)
        if world == 1:  # an identity copy
            assert np.array_equal(order, np.arange(n))


@pytest.mark.parametrize("world", RANKS)
def test_split_without_values(ctx, records, world):
    pid, pk, _ = records
    for n in (65, max(_sizes())):
        _check_split(ctx, pid[:n], pk[:n], None, world)


@pytest.mark.parametrize("world", RANKS)
def test_split_one_destination_gets_everything(ctx, records, world):
    _, pk, val = records
    n = max(_sizes())
    pid = np.full(n, 123456789, dtype=np.int64)
    _check_split(ctx, pid, pk, val, world)
    counts = _split(ctx, pid, pk, val, world)[3]
    assert sorted(counts)[-1] == n and counts.sum() == n


@pytest.mark.parametrize("world", RANKS)
def test_check_shard(ctx, records, world):
    pid = records[0]
    d_pid = torch.from_numpy(pid).cuda()
    n_bad = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    dest = _shard_np(pid, world)
    for rank in sorted({0, world // 2, world - 1}):
        for n in (0, 65, len(pid)):
            ctx.check_shard(d_pid.data_ptr(), n, world, rank, n_bad.data_ptr(), None)
            assert int(n_bad.item()) == int((dest[:n] != rank).sum())
        # a correctly sharded slice: nothing to report
        mine = torch.from_numpy(pid[dest == rank]).cuda()
        ctx.check_shard(mine.data_ptr(), mine.numel(), world, rank, n_bad.data_ptr(), None)
        assert int(n_bad.item()) == 0


@pytest.mark.parametrize("world", [0, 65])
def test_rank_count_out_of_range_raises(ctx, world):
    from pipelinedp_amd import _native
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    counts = torch.zeros(65, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.shard_records(x.data_ptr(), x.data_ptr(), None, 64, world, x.data_ptr(),
                          x.data_ptr(), None, counts.data_ptr(), None)
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.check_shard(x.data_ptr(), 64, world, 0, counts.data_ptr(), None)


def test_two_to_the_31_records_are_unsupported(ctx):
    """Rejected from the arguments alone, like dpg_preaggregate: nothing is
    read or written."""
    from pipelinedp_amd import _native
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError, match="unsupported"):
        ctx.shard_records(x.data_ptr(), x.data_ptr(), None, 1 << 31, 2, x.data_ptr(),
                          x.data_ptr(), None, x.data_ptr(), None)
