"""ColumnarData(sparse_partition_keys=True) through DPEngine on two ranks that
share GPU 0 (gloo process group, as tests/test_gpu_multirank.py) and in one
process.  The two ranks build one key dictionary; for the same seed and nonce
their release equals the one-process release of the same records under the
dictionary's ids given as dense ids (ColumnarData(n_partitions=P)): merged
partials, kept key set, noised values.  The results carry the caller's keys.

One pair of worker processes runs every two-rank release of this module (the
private release, the public one with a rank that holds no record, the
round-robin split with sharding='shuffle', the errors), each a release of its
own; a release that raises is reported to the test that checks it."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SEED, NONCE = 0x5A125E, 0x600DF00D
WORLD = 2
N, N_PID, N_KEYS, N_ABSENT = 200_000, 20_000, 5_000, 50
I64_MIN = -(1 << 63)


def _dataset():
    """Records ordered shard by shard (rank r holds one contiguous block, its
    record ids are offset + i) over about 5 000 sparse keys of either sign."""
    from pipelinedp_amd import distributed
    rng = np.random.default_rng(2024)
    pool = np.unique(rng.integers(-(1 << 62), 1 << 62, N_KEYS + 100, dtype=np.int64))[:N_KEYS]
    rng.shuffle(pool)
    pid = rng.integers(0, N_PID, N).astype(np.int64)
    pk = pool[(rng.zipf(1.1, N) - 1) % N_KEYS]
    val = rng.uniform(-1.0, 11.0, N)
    shard = distributed.shard_of(torch.as_tensor(pid), WORLD).numpy()
    order = np.argsort(shard, kind="stable")
    starts = np.searchsorted(shard[order], np.arange(WORLD + 1))
    return pid[order], pk[order], val[order], starts


def _public_keys():
    """300 keys of the data and 50 keys that no record holds."""
    _, pk, _, _ = _dataset()
    present = np.unique(pk)
    absent = (np.arange(N_ABSENT, dtype=np.int64) - 25) * 1_000_003 + 17
    assert not np.isin(absent, present).any()
    return np.concatenate([present[::len(present) // 300][:300], absent])


def _params(metrics=None):
    import pipelinedp_amd as pdp
    return pdp.AggregateParams(
        metrics=metrics or [pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        max_partitions_contributed=3, max_contributions_per_partition=2,
        min_value=0.0, max_value=10.0)


def _release(pid, pk, val, group, public=None, noise=True, **cols):
    """One release; everything the tests compare, as numpy."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd import columnar
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    data = pdp.ColumnarData(pid=torch.from_numpy(pid).cuda(), pk=torch.from_numpy(pk).cuda(),
                            value=torch.from_numpy(val).cuda(), **cols)
    res = pdp.DPEngine(acc, backend).aggregate(data, _params(),
                                               pdp.DataExtractors("pid", "pk", "value"),
                                               public_partitions=public)
    acc.compute_budgets()
    res.nonce = NONCE
    res.noise_enabled = noise
    out = res.materialize()
    part, lo, stride, n = res.last_slice
    kd = res.last_key_dictionary
    ids = out.partition_ids.cpu().numpy()
    return dict(
        lo=lo, stride=stride, n=n,
        part={k: v.cpu().numpy() for k, v in part.items() if v is not None},
        ids=ids, keys=columnar.decode_keys(ids, out.key_table),
        vals=out.values.cpu().numpy(),
        kd=None if kd is None else dict(
            P=kd.n_partitions, keys=kd.keys.cpu().numpy(), key_ids=kd.key_ids.cpu().numpy(),
            owned=kd.owned_keys.cpu().numpy(), ids=kd.ids.cpu().numpy()))


def _guarded(fn):
    try:
        return ("ok", fn())
    except Exception as e:  # reported to the parent, which asserts on it
        return (type(e).__name__, str(e))


def _worker(rank, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        g = dist.group.WORLD
        pid, pk, val, starts = _dataset()
        a, b = starts[rank], starts[rank + 1]
        out = {}
        out["private"] = _guarded(lambda: _release(
            pid[a:b], pk[a:b], val[a:b], g, sparse_partition_keys=True, record_id_offset=int(a)))
        # rank 1 holds no record
        e = len(pid) if rank == 0 else 0
        out["public"] = _guarded(lambda: _release(
            pid[:e], pk[:e], val[:e], g, public=_public_keys().tolist(), noise=False,
            sparse_partition_keys=True))
        out["shuffle"] = _guarded(lambda: _release(
            pid[rank::WORLD], pk[rank::WORLD], val[rank::WORLD], g, sparse_partition_keys=True,
            sharding="shuffle"))
        bad = pk[a:b].copy()
        if rank == 0:
            bad[5] = I64_MIN  # on one rank only: every rank raises
        out["reserved"] = _guarded(lambda: _release(pid[a:b], bad, val[a:b], g,
                                                    sparse_partition_keys=True))
        out["no_flag"] = _guarded(lambda: _release(pid[a:b], pk[a:b], val[a:b], g))
        out["too_small"] = _guarded(lambda: _release(
            pid[a:b], pk[a:b], val[a:b], g, sparse_partition_keys=True,
            max_distinct_partition_keys=16))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def ranks(built):
    """[rank] -> {release name: ('ok', result) or (error class name, message)}."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=150) for _ in range(WORLD)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return [out for _, out in res]


def _ok(ranks, name):
    for r in ranks:
        assert r[name][0] == "ok", r[name]
    return [r[name][1] for r in ranks]


def _key_ids(results):
    """key -> id over the ranks' dictionaries (one id per key), and P."""
    P = results[0]["kd"]["P"]
    table = {}
    for r in results:
        assert r["kd"]["P"] == P
        for k, i in zip(r["kd"]["keys"].tolist(), r["kd"]["key_ids"].tolist()):
            assert table.setdefault(k, i) == i
    assert len(set(table.values())) == len(table)
    return table, P


@pytest.fixture(scope="module")
def dense(ranks):
    """The one-process dense release of the whole dataset under the ids of the
    two ranks' dictionary: computed once, read by the tests below."""
    results = _ok(ranks, "private")
    table, P = _key_ids(results)
    pid, pk, val, _ = _dataset()
    keys = np.fromiter(table.keys(), np.int64, len(table))
    ids = np.fromiter(table.values(), np.int64, len(table))
    o = np.argsort(keys)
    dense_pk = ids[o][np.searchsorted(keys[o], pk)]
    one = _release(pid, dense_pk, val, None, n_partitions=P)
    id_to_key = np.zeros(P, np.int64)
    id_to_key[ids] = keys
    return one, id_to_key, P, len(table)


def test_private_release_equals_dense_one_process(ranks, dense):
    from pipelinedp_amd import columnar, distributed
    results = _ok(ranks, "private")
    one, id_to_key, P, distinct = dense
    assert (one["lo"], one["stride"], one["n"]) == (0, 1, P)
    assert distinct == len(np.unique(_dataset()[1])) and P % WORLD == 0 and P >= distinct
    want_keys = columnar.decode_keys(one["ids"], id_to_key)
    o1 = np.argsort(np.asarray(want_keys, dtype=np.int64))
    for rank, r in enumerate(results):
        assert (r["lo"], r["stride"], r["n"]) == (rank, WORLD, P // WORLD)
        own = np.arange(rank, P, WORLD)
        assert np.array_equal(r["part"]["rows"], one["part"]["rows"][own])
        assert np.array_equal(r["part"]["count"], one["part"]["count"][own])
        # the dictionary: id % R is the key's owner, id // R its place in the owner's keys
        kd = r["kd"]
        assert np.array_equal(kd["key_ids"] % WORLD,
                              distributed.key_owner(torch.from_numpy(kd["keys"]), WORLD).numpy())
        assert np.array_equal(kd["owned"], id_to_key[own][:len(kd["owned"])])
        # every rank holds the gathered release, keyed by the caller's keys
        assert sorted(r["keys"]) == sorted(want_keys)
        o = np.argsort(r["ids"])
        assert np.array_equal(r["ids"][o], np.asarray(want_keys, dtype=np.int64)[o1])
        assert np.allclose(r["vals"][o], one["vals"][o1], rtol=1e-12, atol=1e-6)
    assert 0 < len(want_keys) < distinct
    assert min(want_keys) < 0 < max(want_keys)


def test_public_partitions_and_a_rank_without_records(ranks):
    results = _ok(ranks, "public")
    public = _public_keys()
    assert results[1]["kd"]["ids"].size == 0  # rank 1 held no record
    for r in results:
        # every public key exactly once, nothing else
        assert sorted(r["keys"]) == sorted(public.tolist())
        assert r["vals"].shape == (len(public), 3)
    # noise off: the keys that no record holds are released empty, the others are not
    r = results[0]
    absent = np.isin(r["ids"], public[-N_ABSENT:])
    assert absent.sum() == N_ABSENT
    # (a present key may still lose all its records to the contribution bounding)
    assert (r["vals"][absent] == 0).all() and (r["vals"][~absent][:, [0, 2]] >= 0).all()
    assert r["vals"][~absent, 2].sum() > 0


def test_shuffled_round_robin_split(ranks):
    first = _ok(ranks, "private")
    results = _ok(ranks, "shuffle")
    for a, b in zip(first, results):
        assert np.array_equal(a["kd"]["owned"], b["kd"]["owned"]) and a["kd"]["P"] == b["kd"]["P"]
        assert np.array_equal(a["part"]["rows"], b["part"]["rows"])
        assert sorted(a["keys"]) == sorted(b["keys"])


def test_one_process_flag_equals_default_encoding(built):
    """Same ids, so the same draws: keys and values are exactly equal.  The
    values are integers: a partition's float sum is accumulated in an order that
    is not fixed from run to run, and only sums of integers do not depend on it."""
    pid, pk, val, _ = _dataset()
    val = np.floor(val)
    flagged = _release(pid, pk, val, None, sparse_partition_keys=True)
    default = _release(pid, pk, val, None)
    assert flagged["kd"] is not None and default["kd"] is None
    assert flagged["kd"]["P"] == len(np.unique(pk))
    assert np.array_equal(flagged["kd"]["ids"], np.unique(pk, return_inverse=True)[1])
    o, o1 = np.argsort(flagged["ids"]), np.argsort(np.asarray(default["keys"], dtype=np.int64))
    assert flagged["keys"] == flagged["ids"].tolist()
    assert np.array_equal(flagged["ids"][o], np.asarray(default["keys"], dtype=np.int64)[o1])
    assert np.array_equal(flagged["vals"][o], default["vals"][o1])
    for k in ("rows", "count", "sum"):
        assert np.array_equal(flagged["part"][k], default["part"][k])
    assert 0 < len(flagged["keys"]) < flagged["kd"]["P"]


def test_one_process_select_partitions_and_public_keys(built):
    """select_partitions yields the caller's keys; public partitions given as a
    tensor, some absent from the data, come out exactly once."""
    import pipelinedp_amd as pdp
    pid, pk, val, _ = _dataset()
    backend = pdp.MI355XBackend(device=0, seed=SEED)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    data = pdp.ColumnarData(pid=torch.from_numpy(pid), pk=pk, sparse_partition_keys=True)
    sel = pdp.DPEngine(acc, backend).select_partitions(
        data, pdp.SelectPartitionsParams(max_partitions_contributed=3),
        pdp.DataExtractors("pid", "pk"))
    acc.compute_budgets()
    got = list(sel)
    assert 0 < len(got) == len(set(got)) < N_KEYS and set(got) <= set(np.unique(pk).tolist())
    public = _public_keys()
    r = _release(pid, pk, val, None, public=torch.from_numpy(public), sparse_partition_keys=True)
    assert sorted(r["keys"]) == sorted(public.tolist())


def test_errors_on_two_ranks(ranks):
    from pipelinedp_amd import distributed
    for r in ranks:
        assert r["reserved"][0] == "ValueError" and "INT64_MIN" in r["reserved"][1]
        assert r["no_flag"] == ("ValueError", distributed.DENSE_IDS_ERROR)
        assert r["too_small"][0] == "ValueError"
        assert "max_distinct" in r["too_small"][1]


def test_errors_in_one_process(built):
    import pipelinedp_amd as pdp
    pid, pk, val, _ = _dataset()
    with pytest.raises(ValueError, match="INT64_MIN"):
        bad = pk.copy()
        bad[7] = I64_MIN
        _release(pid, bad, val, None, sparse_partition_keys=True)
    with pytest.raises(ValueError, match="n_partitions"):
        _release(pid, pk, val, None, sparse_partition_keys=True, n_partitions=10)
    ex = pdp.DataExtractors("pid", "pk", "value")

    def aggregate(data, params=None, public=None, **backend):
        acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
        res = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=SEED, **backend)).aggregate(
            data, params or _params(), ex, public_partitions=public)
        acc.compute_budgets()
        return res.materialize()

    small = slice(0, 1000)
    with pytest.raises(TypeError, match="integer"):  # non-integer keys
        aggregate(pdp.ColumnarData(pid=pid[small], pk=pk[small].astype(np.float64),
                                   value=val[small], sparse_partition_keys=True))
    with pytest.raises(TypeError, match="integer"):
        aggregate(pdp.ColumnarData(pid=pid[small], pk=[str(k) for k in pk[small]],
                                   value=val[small], sparse_partition_keys=True))
    with pytest.raises(TypeError, match="public"):  # non-integer public partitions
        aggregate(pdp.ColumnarData(pid=pid[small], pk=pk[small], value=val[small],
                                   sparse_partition_keys=True), public=["a", "b"])
    with pytest.raises(NotImplementedError, match="PERCENTILE"):
        aggregate(pdp.ColumnarData(pid=pid[small], pk=pk[small], value=val[small],
                                   sparse_partition_keys=True),
                  _params([pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50)]), percentiles=True)
