"""distributed.exchange_owner_keys on CPU tensors over gloo (world 2 and 3):
every key reaches the rank pk % R re-based to pk // R, in source-rank order
and input order within a source; the payload rows follow their keys.  Keys
are dealt round-robin over the first R - 1 ranks: the last rank sends
nothing and still takes part in every collective."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

N, P, D = 1001, 50, 3


def _dataset(low_bits):
    rng = np.random.default_rng(9 + low_bits)
    pk = rng.integers(0, P, N).astype(np.int64)
    low = rng.integers(0, 1 << low_bits, N).astype(np.int64) if low_bits else np.zeros(N, np.int64)
    return (pk << low_bits) | low, rng.uniform(-1.0, 1.0, (N, D))


def _local(world, rank, low_bits):
    keys, rows = _dataset(low_bits)
    if rank == world - 1:
        return keys[:0], rows[:0]
    return keys[rank::world - 1], rows[rank::world - 1]


def _worker(rank, world, port, low_bits, with_payload, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        keys, rows = _local(world, rank, low_bits)
        # a buffer longer than the count: the tail is not sent
        buf = torch.cat([torch.from_numpy(keys), torch.full((5,), 7 << low_bits)])
        pay = torch.cat([torch.from_numpy(rows), torch.zeros((5, D), dtype=torch.float64)])
        r_keys, r_pay, total = distributed.exchange_owner_keys(
            buf, len(keys), low_bits, dist.group.WORLD, payload=pay if with_payload else None)
        q.put((rank, r_keys.numpy(), None if r_pay is None else r_pay.numpy(), total))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, low_bits, with_payload):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, low_bits, with_payload, q))
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


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("low_bits,with_payload", [(16, False), (0, True)])
def test_exchange_owner_keys_gloo(world, low_bits, with_payload):
    res = _run(world, low_bits, with_payload)
    seen = 0
    for rank, r_keys, r_pay, total in res:
        want_keys, want_rows = [], []
        for src in range(world):  # source by source in rank order, input order within
            keys, rows = _local(world, src, low_bits)
            pk = keys >> low_bits
            sel = pk % world == rank
            want_keys.append(((pk[sel] // world) << low_bits) | (keys[sel] & ((1 << low_bits) - 1)))
            want_rows.append(rows[sel])
        want_keys = np.concatenate(want_keys)
        assert np.array_equal(r_keys, want_keys)
        assert total == len(want_keys) > 0
        if with_payload:
            assert np.array_equal(r_pay, np.concatenate(want_rows))
        else:
            assert r_pay is None
        assert ((r_keys >> low_bits) < (P - rank + world - 1) // world).all()
        seen += total
    assert seen == N
