"""distributed.shuffle_records on CPU tensors over gloo (world 2 and 3): every
record reaches the rank shard_of(pid, R), in source-rank order and input
order within a source.  Records are dealt round-robin, the last rank holds
none, and the privacy ids are chosen so that one destination receives
nothing."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

N = 1001


def _shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (pid.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


def _dataset(world):
    """Privacy ids none of which hashes to destination 0."""
    rng = np.random.default_rng(5)
    cand = np.concatenate([rng.integers(-2**40, 2**40, 8 * N),
                           np.array([-1, 2**32 - 1, 2**32, np.iinfo(np.int64).min,
                                     np.iinfo(np.int64).max])]).astype(np.int64)
    pool = cand[_shard_np(cand, world) != 0][:200]
    pid = pool[rng.integers(0, len(pool), N)]
    pk = rng.integers(0, 50, N).astype(np.int64)
    val = rng.uniform(-1.0, 11.0, N)
    return pid, pk, val


def _local(world, rank):
    """Round-robin over the first world - 1 ranks; the last rank holds nothing."""
    pid, pk, val = _dataset(world)
    if rank == world - 1:
        return pid[:0], pk[:0], val[:0]
    return pid[rank::world - 1], pk[rank::world - 1], val[rank::world - 1]


def _worker(rank, world, port, with_value, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pid, pk, val = _local(world, rank)
        r_pid, r_pk, r_val = distributed.shuffle_records(
            torch.from_numpy(pid), torch.from_numpy(pk),
            torch.from_numpy(val) if with_value else None, dist.group.WORLD)
        q.put((rank, r_pid.numpy(), r_pk.numpy(), None if r_val is None else r_val.numpy()))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, with_value):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, with_value, q))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=90) for _ in range(world)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return res


def test_shard_of_equals_uint32_form():
    """The device's shard (uint32 multiply, umulhi) is distributed.shard_of."""
    from pipelinedp_amd import distributed
    rng = np.random.default_rng(3)
    pid = np.concatenate([rng.integers(-2**62, 2**62, 5000),
                          np.array([0, -1, 2**32 - 1, 2**32, np.iinfo(np.int64).min,
                                    np.iinfo(np.int64).max])]).astype(np.int64)
    for world in (1, 2, 3, 8, 64):
        got = distributed.shard_of(torch.from_numpy(pid), world).numpy()
        assert np.array_equal(got, _shard_np(pid, world))
        assert got.min() >= 0 and got.max() < world


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("with_value", [True, False])
def test_shuffle_records_gloo(world, with_value):
    res = _run(world, with_value)
    pid, pk, val = _dataset(world)
    got_pid, got_pk, got_val = [], [], []
    for rank, r_pid, r_pk, r_val in res:
        # destination `rank`: source by source in rank order, input order within
        want = [[], [], []]
        for src in range(world):
            s_pid, s_pk, s_val = _local(world, src)
            sel = _shard_np(s_pid, world) == rank
            for col, s in zip(want, (s_pid, s_pk, s_val)):
                col.append(s[sel])
        assert np.array_equal(r_pid, np.concatenate(want[0]))
        assert np.array_equal(r_pk, np.concatenate(want[1]))
        if with_value:
            assert np.array_equal(r_val, np.concatenate(want[2]))
        else:
            assert r_val is None
        # every privacy id ends on exactly one rank: its owner
        assert np.all(_shard_np(r_pid, world) == rank)
        got_pid.append(r_pid)
        got_pk.append(r_pk)
        got_val.append(r_val)
    assert len(res[0][1]) == 0  # the destination nobody hashes to
    # the union over ranks is a permutation of the input
    a_pid, a_pk = np.concatenate(got_pid), np.concatenate(got_pk)
    assert len(a_pid) == N
    if with_value:
        a_val = np.concatenate(got_val)
        o, o0 = np.lexsort((a_val, a_pk, a_pid)), np.lexsort((val, pk, pid))
        assert np.array_equal(a_val[o], val[o0])
    else:
        o, o0 = np.lexsort((a_pk, a_pid)), np.lexsort((pk, pid))
    assert np.array_equal(a_pid[o], pid[o0]) and np.array_equal(a_pk[o], pk[o0])


def test_sharding_field_is_validated():
    import pipelinedp_amd as pdp
    assert pdp.ColumnarData().sharding == "trusted"
    for mode in ("trusted", "verify", "shuffle"):
        assert pdp.ColumnarData(sharding=mode).sharding == mode
    with pytest.raises(ValueError, match="sharding"):
        pdp.ColumnarData(sharding="sorted")
