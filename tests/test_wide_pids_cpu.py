"""Wide privacy ids without a GPU: distributed.shard_of_wide is key_owner;
distributed.encode_privacy_ids on CPU tensors over gloo (world 2 and 3) gives
every rank the ascending ranks of its own ids, raises a reserved id or an
overflow of one rank on all ranks, and takes a rank without records along;
shuffle_records' host fallback delivers by shard_of_wide; ColumnarData and
columnar.encode validate the flag."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1
N_PER_RANK, N_IDS = 3000, 400
CASES = ("plain", "empty", "reserved", "overflow", "roomy", "shuffle")


def _fmix64(k: int) -> int:
    k &= M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def test_shard_of_wide_is_key_owner():
    from pipelinedp_amd import distributed
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(I64_MIN, I64_MAX, 500, dtype=np.int64, endpoint=True),
                          np.array([0, -1, 1, I64_MAX, I64_MIN, 1 << 32, (1 << 32) - 1],
                                   dtype=np.int64),
                          np.arange(1, 200, dtype=np.int64) << 32])
    t = torch.from_numpy(ids)
    for world in (1, 2, 3, 7, 8, 64):
        got = distributed.shard_of_wide(t, world)
        assert torch.equal(got, distributed.key_owner(t, world))
        want = [((_fmix64(int(k)) >> 32) * world) >> 32 for k in ids]
        assert got.tolist() == want
    # ids that differ only above bit 31: the narrow function sees one id
    high = t[-199:]
    assert len(torch.unique(distributed.shard_of(high, 8))) == 1
    assert len(torch.unique(distributed.shard_of_wide(high, 8))) == 8


def _pool():
    rng = np.random.default_rng(43)
    pool = rng.integers(I64_MIN + 1, I64_MAX, N_IDS - 5, dtype=np.int64, endpoint=True)
    return np.unique(np.concatenate([pool, np.array([0, -1, I64_MAX, I64_MIN + 1, 1 << 32],
                                                    dtype=np.int64)]))


def _local(world, rank, case):
    pool = _pool()
    rng = np.random.default_rng(200 + rank)
    pid = pool[rng.integers(0, len(pool), N_PER_RANK)]
    if case == "empty" and rank == world - 1:
        pid = pid[:0]
    if case == "reserved" and rank == 0:
        pid = pid.copy()
        pid[17] = I64_MIN
    if case == "overflow" and rank != 0:
        pid = pid[:20] * 0 + pid[0]  # one id: only rank 0 overflows its table
    return pid


def _enc(pid, max_distinct=None):
    from pipelinedp_amd import columnar
    t = torch.from_numpy(np.ascontiguousarray(pid))
    return columnar.EncodedInput(pid=t, pk=torch.zeros(len(pid), dtype=torch.int64), value=None,
                                 n=len(pid), n_partitions=1, key_table=None, pid_unencoded=True,
                                 pid_wide=True, max_distinct_pids=max_distinct)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        backend = types.SimpleNamespace(world_size=world, process_group=dist.group.WORLD,
                                        device=torch.device("cpu"))
        out = {}
        for case in CASES:
            pid = _local(world, rank, case)
            if case == "shuffle":
                pk = torch.arange(len(pid), dtype=torch.int64) + rank * N_PER_RANK
                val = pk.to(torch.float64) * 0.5
                r = distributed.shuffle_records(torch.from_numpy(pid), pk, val,
                                                dist.group.WORLD, wide=True)
                out[case] = ("ok", [x.numpy() for x in r])
                continue
            md = {"overflow": 16, "roomy": N_IDS}.get(case)
            enc = _enc(pid, md)
            try:
                distributed.encode_privacy_ids(enc, backend)
                out[case] = ("ok", enc.pid.numpy(), enc.pid_min, enc.pid_count, enc.pid_wide)
            except ValueError as e:
                out[case] = ("ValueError", str(e))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request):
    """(world, [rank] -> {case: outcome}): one set of workers per world size
    runs every case."""
    world = request.param
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
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
    return world, [out for _, out in res]


@pytest.mark.parametrize("case", ["plain", "empty", "roomy"])
def test_ids_are_the_local_ascending_ranks(ranks, case):
    world, outs = ranks
    for rank, out in enumerate(outs):
        status, ids, pid_min, pid_count, still_wide = out[case]
        assert status == "ok"
        pid = _local(world, rank, case)
        uniq, inv = np.unique(pid, return_inverse=True)
        assert ids.dtype == np.int64 and np.array_equal(ids, inv)
        assert (pid_min, pid_count, still_wide) == (0, max(1, len(uniq)), False)
    if case == "empty":  # the rank without records took part and got nothing
        assert outs[-1][case][1].size == 0 and outs[-1][case][3] == 1


def test_reserved_id_on_one_rank_raises_on_all(ranks):
    _, outs = ranks
    for out in outs:
        assert out["reserved"][0] == "ValueError"
        assert "1 records hold the privacy id INT64_MIN" in out["reserved"][1]
    assert len({out["reserved"][1] for out in outs}) == 1


def test_overflow_on_one_rank_raises_on_all(ranks):
    world, outs = ranks
    distinct = len(np.unique(_local(world, 0, "overflow")))
    assert distinct > 64  # the table of max_distinct_privacy_ids=16 has 64 slots
    for out in outs:
        assert out["overflow"][0] == "ValueError"
        assert "max_distinct_privacy_ids=16" in out["overflow"][1]
    assert len({out["overflow"][1] for out in outs}) == 1


def test_host_shuffle_delivers_by_shard_of_wide(ranks):
    from pipelinedp_amd import distributed
    world, outs = ranks
    sent = [_local(world, r, "shuffle") for r in range(world)]
    for rank, out in enumerate(outs):
        pid, pk, val = out["shuffle"][1]
        # source-rank order, input order within a source
        want_pid, want_pk = [], []
        for src in range(world):
            mine = distributed.shard_of_wide(torch.from_numpy(sent[src]), world).numpy() == rank
            want_pid.append(sent[src][mine])
            want_pk.append(np.arange(N_PER_RANK)[mine] + src * N_PER_RANK)
        assert np.array_equal(pid, np.concatenate(want_pid))
        assert np.array_equal(pk, np.concatenate(want_pk))
        assert np.array_equal(val, pk * 0.5)
    assert sum(len(out["shuffle"][1][0]) for out in outs) == world * N_PER_RANK


def test_one_process_on_host_tensors():
    from pipelinedp_amd import distributed
    backend = types.SimpleNamespace(world_size=1, process_group=None, device=torch.device("cpu"))
    pid = _local(1, 0, "plain")
    enc = _enc(pid)
    distributed.encode_privacy_ids(enc, backend)
    uniq, inv = np.unique(pid, return_inverse=True)
    assert np.array_equal(enc.pid.numpy(), inv) and enc.pid_count == len(uniq)
    with pytest.raises(ValueError, match="INT64_MIN"):
        distributed.encode_privacy_ids(_enc(_local(1, 0, "reserved")), backend)
    with pytest.raises(ValueError, match="max_distinct_privacy_ids=16"):
        distributed.encode_privacy_ids(_enc(pid, 16), backend)
    # an input that is not marked is left alone
    enc = _enc(pid)
    enc.pid_wide = False
    distributed.encode_privacy_ids(enc, backend)
    assert np.array_equal(enc.pid.numpy(), pid) and enc.pid_count == 0


def test_table_capacity():
    from pipelinedp_amd import distributed
    cap = distributed._pid_capacity
    assert [cap(n, None) for n in (0, 1, 32, 33, 1000)] == [64, 64, 64, 128, 2048]
    assert cap(10**9, 10**7) == 1 << 25 and cap(100, 10**7) == 256
    assert cap((1 << 31) - 1, None) == 1 << 31  # the table calls' limit


def test_columnar_data_validation():
    import pipelinedp_amd as pdp
    from pipelinedp_amd import columnar
    pid = np.array([1 << 40, -(1 << 50), 7, 1 << 40], dtype=np.int64)
    pk = np.array([0, 1, 1, 2], dtype=np.int64)
    with pytest.raises(ValueError, match="privacy_id_range"):
        pdp.ColumnarData(pid=pid, pk=pk, wide_privacy_ids=True, privacy_id_range=(0, 10))
    with pytest.raises(TypeError, match="needs integers"):
        pdp.ColumnarData(pid=pid.astype(np.float64), pk=pk, wide_privacy_ids=True)
    with pytest.raises(TypeError, match="needs integers"):
        pdp.ColumnarData(pid=torch.from_numpy(pid).to(torch.float32), pk=pk,
                         wide_privacy_ids=True)
    with pytest.raises(TypeError, match="needs integers"):
        pdp.ColumnarData(pid=["a", "b", "c", "d"], pk=pk, wide_privacy_ids=True)
    ex = pdp.DataExtractors("pid", "pk", "value")
    cpu = torch.device("cpu")
    for hint in (None, 3):
        col = pdp.ColumnarData(pid=pid, pk=pk, value=np.ones(4), n_partitions=hint,
                               wide_privacy_ids=True, max_distinct_privacy_ids=9)
        enc = columnar.encode(col, ex, cpu, True)
        # the ids stay the caller's; the input is marked for encode_privacy_ids
        assert enc.pid.dtype == torch.int64 and np.array_equal(enc.pid.numpy(), pid)
        assert enc.pid_wide and enc.pid_unencoded and not enc.pid_range_declared
        assert (enc.pid_min, enc.pid_count, enc.max_distinct_pids) == (0, 0, 9)
    # a column that an extractor produces is checked when it is encoded
    col = pdp.ColumnarData(pid=pid, pk=pk, value=np.ones(4), wide_privacy_ids=True)
    with pytest.raises(TypeError, match="needs integers"):
        columnar.encode(col, pdp.DataExtractors(lambda c: c.pid * 0.5, "pk", "value"), cpu, True)
    # the privacy ids are not read: the flag does nothing
    enc = columnar.encode(col, ex, cpu, True, need_pid=False)
    assert enc.pid is None and not enc.pid_wide
    # the flag off: the default encoding, unmarked
    enc = columnar.encode(pdp.ColumnarData(pid=pid, pk=pk, value=np.ones(4)), ex, cpu, True)
    assert not enc.pid_wide and enc.pid_count == 3 and enc.pid.tolist() == [2, 0, 1, 2]
