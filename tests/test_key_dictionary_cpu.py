"""distributed.build_key_dictionary on CPU tensors over gloo (world 2 and 3)
and in one process: sparse int64 partition keys get global dense ids that are
the same on every rank, whose owner is id % R and whose position in the
owner's sorted keys is id // R; the errors are raised on every rank alike.
key_hash / key_owner are checked against a hand-written fmix64."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1
N_PER_RANK, N_KEYS, N_PUBLIC = 3000, 500, 40


def _fmix64(k: int) -> int:
    k &= M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def _owner(k: int, world: int) -> int:
    return ((_fmix64(k) >> 32) * world) >> 32


def _key_pool():
    """About 500 distinct keys over the whole int64 range, the extremes among them."""
    rng = np.random.default_rng(41)
    pool = rng.integers(I64_MIN + 1, I64_MAX, N_KEYS - 6, dtype=np.int64, endpoint=True)
    return np.unique(np.concatenate([pool, np.array([0, -1, 1, I64_MAX, I64_MIN + 1, -12345],
                                                    dtype=np.int64)]))


def _public():
    """Public keys: 20 of the pool and 20 that no record holds."""
    pool = _key_pool()
    absent = np.arange(20, dtype=np.int64) * 7919 + (1 << 40)
    assert not np.isin(absent, pool).any()
    return np.concatenate([pool[::len(pool) // 20][:20], absent])


def _local(world, rank, case):
    """This rank's record keys.  'empty': the last rank holds no record."""
    pool = _key_pool()
    rng = np.random.default_rng(100 + rank)
    pk = pool[rng.integers(0, len(pool), N_PER_RANK)]
    if case == "empty" and rank == world - 1:
        pk = pk[:0]
    if case == "reserved" and rank == 0:
        pk = pk.copy()
        pk[17] = I64_MIN
    return pk


def _worker(rank, world, port, case, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pk = torch.from_numpy(_local(world, rank, case))
        public = torch.from_numpy(_public()) if case in ("public", "empty") else None
        out = []
        for _ in range(2):  # two runs: identical ids
            try:
                kd = distributed.build_key_dictionary(
                    pk, public, dist.group.WORLD,
                    max_distinct=10 if case == "overflow" else None)
                out.append(("ok", kd.ids.numpy(),
                            None if kd.public_ids is None else kd.public_ids.numpy(),
                            kd.n_partitions, kd.owned_keys.numpy(), kd.keys.numpy(),
                            kd.key_ids.numpy()))
            except ValueError as e:
                out.append(("ValueError", str(e)))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
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
    return [out for _, out in res]


def test_key_hash_matches_fmix64():
    from pipelinedp_amd import distributed
    keys = [0, 1, -1, 2, 42, -42, I64_MAX, I64_MIN + 1, I64_MIN, 0x0123456789ABCDEF,
            -0x0123456789ABCDEF, 1 << 32, (1 << 33) - 1, -(1 << 33)]
    # fixed vectors of murmur3's finaliser, so that the hand-written mirror is pinned too
    assert _fmix64(0) == 0
    assert _fmix64(1) == 0xb456bcfc34c2cb2c
    got = distributed.key_hash(torch.tensor(keys, dtype=torch.int64)).tolist()
    assert [g & M64 for g in got] == [_fmix64(k) for k in keys]
    for world in (1, 2, 3, 7, 64):
        own = distributed.key_owner(torch.tensor(keys, dtype=torch.int64), world).tolist()
        assert own == [_owner(k, world) for k in keys]
        assert all(0 <= o < world for o in own)


def _check_dictionary(world, case, res):
    key_id = {}
    P = res[0][0][3]
    owned_all = []
    for rank, runs in enumerate(res):
        first, second = runs
        assert first[0] == second[0] == "ok"
        for a, b in zip(first[1:], second[1:]):  # two runs give identical results
            assert (a is None and b is None) or np.array_equal(a, b)
        _, ids, public_ids, P_r, owned, keys, key_ids = first
        assert P_r == P
        pk = _local(world, rank, case)
        assert ids.shape == pk.shape and ids.dtype == np.int64
        assert np.array_equal(owned, np.unique(owned)) and owned.dtype == np.int64
        assert all(_owner(int(k), world) == rank for k in owned)
        owned_all.append(owned)
        pairs = list(zip(pk.tolist(), ids.tolist()))
        if public_ids is not None:
            pairs += list(zip(_public().tolist(), public_ids.tolist()))
        want = np.unique(np.concatenate([pk] + ([_public()] if public_ids is not None else [])))
        assert np.array_equal(keys, want)
        pairs += list(zip(keys.tolist(), key_ids.tolist()))
        for k, i in pairs:
            assert key_id.setdefault(k, i) == i  # one key, one id, on every rank
            assert 0 <= i < P
            assert i % world == _owner(k, world)
            assert owned[i // world] == k if i % world == rank else True
    # distinct keys map to distinct ids
    assert len(set(key_id.values())) == len(key_id)
    assert P == world * max(len(o) for o in owned_all)
    for k, i in key_id.items():
        assert owned_all[i % world][i // world] == k
    # the owners hold the union of the key sets, each key once
    union = np.concatenate(owned_all)
    assert len(union) == len(key_id) and set(union.tolist()) == set(key_id)
    return key_id


@pytest.mark.parametrize("world", [2, 3])
def test_ids_are_global_dense_and_owned(world):
    key_id = _check_dictionary(world, "plain", _run(world, "plain"))
    for k in (0, -1, I64_MAX, I64_MIN + 1):
        assert k in key_id or k not in _key_pool()
    assert min(key_id) < 0 < max(key_id)


@pytest.mark.parametrize("world", [2, 3])
def test_rank_without_records_and_absent_public_keys(world):
    res = _run(world, "empty")
    key_id = _check_dictionary(world, "empty", res)
    assert res[world - 1][0][1].size == 0
    # public keys that no record holds have ids, the same on every rank
    for k in _public().tolist():
        assert k in key_id


@pytest.mark.parametrize("world", [2, 3])
def test_public_keys_get_ids(world):
    key_id = _check_dictionary(world, "public", _run(world, "public"))
    assert all(k in key_id for k in _public().tolist())


@pytest.mark.parametrize("world", [2, 3])
def test_reserved_key_raises_on_every_rank(world):
    for runs in _run(world, "reserved"):
        for kind, msg in runs:
            assert kind == "ValueError" and "INT64_MIN" in msg


@pytest.mark.parametrize("world", [2, 3])
def test_max_distinct_too_small_raises_on_every_rank(world):
    for runs in _run(world, "overflow"):
        for kind, msg in runs:
            assert kind == "ValueError" and "max_distinct" in msg


def test_one_process_ids_equal_np_unique():
    from pipelinedp_amd import distributed
    pk = _local(1, 0, "plain")
    public = _public()
    kd = distributed.build_key_dictionary(torch.from_numpy(pk), torch.from_numpy(public), None)
    uniq, inv = np.unique(np.concatenate([pk, public]), return_inverse=True)
    assert np.array_equal(kd.ids.numpy(), inv[:len(pk)])
    assert np.array_equal(kd.public_ids.numpy(), inv[len(pk):])
    assert kd.n_partitions == len(uniq)
    assert np.array_equal(kd.owned_keys.numpy(), uniq)
    assert np.array_equal(kd.keys.numpy(), uniq)
    assert np.array_equal(kd.key_ids.numpy(), np.arange(len(uniq)))
    kd = distributed.build_key_dictionary(torch.from_numpy(pk), None, None)
    assert np.array_equal(kd.ids.numpy(), np.unique(pk, return_inverse=True)[1])
    assert kd.public_ids is None
    with pytest.raises(ValueError, match="INT64_MIN"):
        distributed.build_key_dictionary(torch.tensor([3, I64_MIN, 5]), None, None)


def test_columnar_flag_checks():
    """The ColumnarData fields: defaults off; the flag refuses n_partitions."""
    from pipelinedp_amd import columnar
    c = columnar.ColumnarData(pk=[1, 2])
    assert c.sparse_partition_keys is False and c.max_distinct_partition_keys is None
    with pytest.raises(ValueError, match="n_partitions"):
        columnar.ColumnarData(pk=[1, 2], n_partitions=4, sparse_partition_keys=True)
