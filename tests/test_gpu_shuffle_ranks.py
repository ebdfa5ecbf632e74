"""ColumnarData(sharding=...) with two gloo ranks on GPU 0 (as
test_gpu_multirank.py: RCCL refuses two ranks on one device).  Rank r gets
the records r::2, so nearly every privacy id sits on both ranks:

* "shuffle": rows, count and the kept set equal the one-process release of
  the whole dataset; sum equals the release of what each rank received;
* "verify": both ranks raise ValueError and exit by themselves; on a
  shard_of-sorted split the release equals the "trusted" one exactly;
* string privacy ids with "shuffle" raise ValueError on every rank."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SEED, NONCE, P = 0xAB5EED, 0x1234ABCD, 3_000
WORLD = 2


def _shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (pid.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


def _dataset():
    rng = np.random.default_rng(12)
    n = 60_000
    pid = rng.integers(0, 4_000, n).astype(np.int64)
    pk = ((rng.zipf(1.1, n) - 1) % P).astype(np.int64)
    val = rng.uniform(-1.0, 11.0, n)
    return pid, pk, val


def _sorted_split(rank):
    """Rank's block of the shard_of-sorted dataset and its record id offset."""
    pid, pk, val = _dataset()
    shard = _shard_np(pid, WORLD)
    order = np.argsort(shard, kind="stable")
    starts = np.searchsorted(shard[order], np.arange(WORLD + 1))
    sel = order[starts[rank]:starts[rank + 1]]
    return pid[sel], pk[sel], val[sel], int(starts[rank])


def _params():
    import pipelinedp_amd as pdp
    return pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        max_partitions_contributed=3, max_contributions_per_partition=2,
        min_value=0.0, max_value=10.0)


def _release(pid, pk, val, offset, group, sharding="trusted"):
    import pipelinedp_amd as pdp
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    if isinstance(pid, np.ndarray) and pid.dtype.kind in "iu":
        pid = torch.from_numpy(pid).cuda()
    cols = pdp.ColumnarData(pid=pid, pk=torch.from_numpy(pk).cuda(),
                            value=torch.from_numpy(val).cuda(), n_partitions=P,
                            record_id_offset=int(offset), sharding=sharding)
    res = pdp.DPEngine(acc, backend).aggregate(cols, _params(),
                                               pdp.DataExtractors("pid", "pk", "value"))
    acc.compute_budgets()
    res.nonce = NONCE
    out = res.materialize()
    part, lo, stride, n = res.last_slice
    return (lo, stride, n, {k: v.cpu().numpy() for k, v in part.items() if v is not None},
            out.partition_ids.cpu().numpy(), out.values.cpu().numpy())


def _worker(rank, port, case, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        pid, pk, val = _dataset()
        pid, pk, val, offset = pid[rank::WORLD], pk[rank::WORLD], val[rank::WORLD], 0
        try:
            if case == "shuffle":
                got = _release(pid, pk, val, 0, dist.group.WORLD, "shuffle")
            elif case == "verify_bad":
                got = _release(pid, pk, val, 0, dist.group.WORLD, "verify")
            elif case == "verify_good":
                pid, pk, val, offset = _sorted_split(rank)
                got = (_release(pid, pk, val, offset, dist.group.WORLD, "verify"),
                       _release(pid, pk, val, offset, dist.group.WORLD, "trusted"))
            elif case == "string_pid":
                names = np.array([f"user{p}" for p in pid])
                got = _release(names, pk, val, 0, dist.group.WORLD, "shuffle")
            q.put((rank, "ok", got))
        except ValueError as e:
            q.put((rank, "ValueError", str(e)))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, case, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=100) for _ in range(WORLD)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return res


@pytest.fixture(scope="module")
def one_rank(built):
    """The one-process release of the whole dataset."""
    pid, pk, val = _dataset()
    return _release(pid, pk, val, 0, None)


def test_shuffle_equals_one_rank(built, one_rank):
    res = _run("shuffle")
    lo1, s1, n1, full, ids1, _ = one_rank
    assert (lo1, s1, n1) == (0, 1, P)
    # what destination d received: source by source, input order within
    pid, pk, val = _dataset()
    want_sum = np.zeros(P)
    for d in range(WORLD):
        parts = []
        for src in range(WORLD):
            s = [pid[src::WORLD], pk[src::WORLD], val[src::WORLD]]
            sel = _shard_np(s[0], WORLD) == d
            parts.append([c[sel] for c in s])
        got = [np.concatenate([p[i] for p in parts]) for i in range(3)]
        want_sum += _release(got[0], got[1], got[2], 0, None)[3]["sum"]
    for rank, status, got in res:
        assert status == "ok", got
        lo, stride, n, part, ids, vals = got
        assert lo == rank and stride == WORLD and n == P // WORLD
        own = np.arange(rank, P, WORLD)
        assert np.array_equal(part["rows"], full["rows"][own])
        assert np.array_equal(part["count"], full["count"][own])
        assert np.allclose(part["sum"], want_sum[own], rtol=1e-12, atol=1e-9)
        assert np.array_equal(np.sort(ids), np.sort(ids1))
    assert 0 < len(ids1) < P


def test_verify_raises_on_every_rank(built):
    res = _run("verify_bad")
    n_bad = int(sum((_shard_np(_dataset()[0][r::WORLD], WORLD) != r).sum() for r in range(WORLD)))
    assert n_bad > 0
    for rank, status, msg in res:
        assert status == "ValueError", (rank, status)
        assert str(n_bad) in msg


def test_verify_passes_on_a_sharded_split(built):
    res = _run("verify_good")
    for rank, status, got in res:
        assert status == "ok", got
        verified, trusted = got
        assert verified[:3] == trusted[:3]
        # the release: kept ids and released values, exactly
        assert np.array_equal(verified[4], trusted[4])
        assert np.array_equal(verified[5], trusted[5])
        assert len(trusted[4]) > 0
        # the partials behind it: integers exactly; the float sums of two
        # releases of one input differ by their summation order even in one
        # process (measured: ~1e-15 relative in a few dozen partitions), so
        # they take test_gpu_multirank.py's summation-order tolerance
        assert np.array_equal(verified[3]["rows"], trusted[3]["rows"])
        assert np.array_equal(verified[3]["count"], trusted[3]["count"])
        assert np.allclose(verified[3]["sum"], trusted[3]["sum"], rtol=1e-12, atol=1e-9)


def test_string_privacy_ids_raise_on_every_rank(built):
    res = _run("string_pid")
    for rank, status, msg in res:
        assert status == "ValueError", (rank, status)
        assert "integer privacy ids" in msg
