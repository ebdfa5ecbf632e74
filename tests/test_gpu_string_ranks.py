"""ColumnarData(global_string_keys=True) through DPEngine: a StringColumn of
partition keys on two ranks that share GPU 0 (gloo process group, as
tests/test_gpu_string_engine.py, whose dataset this file uses) and in one
process.

The ids of the global string dictionary are known without running it
(tests/string_pack_ref.py: global_ids -- i * R + owner, i the ascending signed
rank of the string's hash among its owner's hashes), so a flagged release must
be, bit for bit, the one-process DENSE release of those ids with n_partitions =
P under the same backend seed and nonce.  The values are integers: a
partition's sum does not depend on the order of its additions."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import string_pack_ref, string_ref
from tests import test_gpu_string_engine as base

SEED, NONCE, WORLD = base.SEED, base.NONCE, base.WORLD
N, N_PK = base.N, base.N_PK
ABSENT = [f"absent from the data/{i} Ω" for i in range(5)]
CONSTANT_KEY = 0x1234_5678_9ABC


def _public():
    return base._names()[0] + ABSENT


def _sharded():
    """The dataset ordered shard by shard under shard_of(pid, WORLD) and the
    blocks' starts: rank r holds [starts[r], starts[r + 1])."""
    from pipelinedp_amd import distributed
    pid_s, pk_s, pid_i, pk_i, val = base._dataset()
    shard = distributed.shard_of(torch.from_numpy(pid_i), WORLD).numpy()
    order = np.argsort(shard, kind="stable")
    starts = np.searchsorted(shard[order], np.arange(WORLD + 1))
    return pid_i[order], [pk_s[i] for i in order], val[order], starts


def _release(pid, pk, val, group=None, public=None, noise=True, binding=True, gather=True,
             **cols):
    """One aggregate release; everything the tests compare."""
    import pipelinedp_amd as pdp
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    data = pdp.ColumnarData(pid=base._cuda(pid), pk=base._cuda(pk), value=base._cuda(val), **cols)
    res = pdp.DPEngine(acc, backend).aggregate(data, base._params(binding=binding),
                                               pdp.DataExtractors("pid", "pk", "value"),
                                               public_partitions=public)
    acc.compute_budgets()
    res.nonce = NONCE
    res.noise_enabled = noise
    try:
        out = res.materialize(gather=gather)
    except Exception:
        assert res.last_bound_fields is None, "raised after bounding had been set up"
        raise
    part, lo, stride, local_P = res.last_slice
    sd = res.last_string_dictionary
    return dict(part={k: v.cpu().numpy() for k, v in part.items() if v is not None},
                slice=(lo, stride, local_P), keys=out.keys(),
                ids=out.partition_ids.cpu().numpy(), vals=out.values.cpu().numpy(),
                P=None if sd is None else sd.n_partitions,
                rec_ids=None if sd is None else sd.ids.cpu().numpy(),
                iterated=[(k, tuple(m)) for k, m in res])


def _select(pid, pk, group=None, **cols):
    import pipelinedp_amd as pdp
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    sel = pdp.DPEngine(acc, backend).select_partitions(
        pdp.ColumnarData(pid=base._cuda(pid), pk=base._cuda(pk), **cols),
        pdp.SelectPartitionsParams(max_partitions_contributed=3), pdp.DataExtractors("pid", "pk"))
    acc.compute_budgets()
    sel.nonce = NONCE
    return list(sel)


def _constant_keys(offsets, data, seed, ctx, stream=None):
    n = offsets.numel() - 1
    return (torch.full((n,), CONSTANT_KEY, dtype=torch.int64, device=offsets.device),
            torch.zeros(1, dtype=torch.int64, device=offsets.device))


def _worker(rank, port, q):
    import pipelinedp_amd as pdp
    import torch.distributed as dist
    from pipelinedp_amd import string_columns
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        g = dist.group.WORLD
        pid, pk_s, val, starts = _sharded()
        a, b = int(starts[rank]), int(starts[rank + 1])
        flag = dict(global_string_keys=True)
        out = {}
        # 1, 3, 4: private selection, binding bounds, noise on
        out["private"] = base._guarded(lambda: _release(
            pid[a:b], base._column(pk_s[a:b]), val[a:b], g, record_id_offset=a, **flag))
        out["owned"] = base._guarded(lambda: _release(
            pid[a:b], base._column(pk_s[a:b]), val[a:b], g, gather=False, record_id_offset=a,
            max_distinct_partition_keys=N_PK, **flag))
        out["select"] = base._guarded(lambda: _select(
            pid[a:b], base._column(pk_s[a:b]), g, record_id_offset=a, **flag))
        # 2: public partitions, rank 1 holds no record
        e = N if rank == 0 else 0
        out["public"] = base._guarded(lambda: _release(
            pid[:e], base._column(pk_s[:e]), val[:e], g, public=_public(), noise=False,
            binding=False, **flag))
        # 5: round-robin split, shuffled; string privacy ids beside the string keys
        r_pid, r_pk, _, _, r_val = base._dataset()
        out["shuffle"] = base._guarded(lambda: _release(
            base._column(r_pid[rank::WORLD]), base._column(r_pk[rank::WORLD]), r_val[rank::WORLD],
            g, public=base._column(_public()), noise=False, binding=False, sharding="shuffle",
            **flag))
        # 6: errors on one rank, or visible to the owner only
        col = base._column(pk_s[a:b])
        if rank == 0:
            col.offsets[3] = -1  # records 2 and 3
        out["bad_offsets"] = base._guarded(lambda: _release(
            pid[a:b], pdp.StringColumn(col.offsets, col.data), val[a:b], g, record_id_offset=a,
            **flag))
        words = ["alpha"] * 50 if rank == 0 else ["beta"] * 30
        real = string_columns.device_keys
        string_columns.device_keys = _constant_keys
        try:
            out["collision"] = base._guarded(lambda: _release(
                np.arange(len(words)), base._column(words), np.ones(len(words)), g, **flag))
        finally:
            string_columns.device_keys = real
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(built):
    """[rank] -> {release name: ('ok', result) or (error class name, message)}."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = base._free_port()
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


@pytest.fixture(scope="module")
def rule():
    """({string: id}, P) of the data's strings on WORLD ranks, from the rule."""
    return string_pack_ref.global_ids(base._names()[0], WORLD)


@pytest.fixture(scope="module")
def dense(built, rule):
    """The one-process dense release of pk = the rule's ids, n_partitions = P,
    over the shard-ordered dataset (record ids = positions, as the ranks'
    record_id_offset gives them); and the same for select_partitions."""
    ids, P = rule
    pid, pk_s, val, _ = _sharded()
    pk = np.array([ids[s] for s in pk_s], dtype=np.int64)
    name = {i: s for s, i in ids.items()}
    one = _release(pid, pk, val, n_partitions=P)
    one["by_string"] = {name[i]: tuple(v) for i, v in zip(one["ids"].tolist(),
                                                          one["vals"].tolist())}
    one["selected"] = sorted(name[i] for i in _select(pid, pk, n_partitions=P))
    return one


def _groupby():
    """{string: (COUNT, SUM of the clipped values, PRIVACY_ID_COUNT)}."""
    pid_s, pk_s, pid_i, pk_i, val = base._dataset()
    want = {s: (0.0, 0.0, 0.0) for s in _public()}
    clipped = np.clip(val, 0.0, 10.0)
    names = base._names()[0]
    for p in np.unique(pk_i):
        m = pk_i == p
        want[names[p]] = (float(m.sum()), float(clipped[m].sum()),
                          float(np.unique(pid_i[m]).size))
    return want


# ------------------------------------------------------------------ two ranks
@pytest.mark.gpu
def test_two_ranks_private_release_equals_dense_release_of_the_ids(ranks, rule, dense):
    ids, P = rule
    results = base._ok(ranks, "private")
    _, pk_s, _, starts = _sharded()
    for rank, r in enumerate(results):
        assert r["P"] == P == WORLD * max(
            len(string_pack_ref.owned_strings(ids, WORLD, k)) for k in range(WORLD))
        local = pk_s[starts[rank]:starts[rank + 1]]
        assert np.array_equal(r["rec_ids"], np.array([ids[s] for s in local]))
        lo, stride, local_P = r["slice"]
        assert (lo, stride) == (rank, WORLD)
        assert set(r["part"]) == set(dense["part"]) == {"rows", "count", "sum"}
        for k in r["part"]:  # this rank's merged slice of the partials
            assert np.array_equal(r["part"][k][:local_P], dense["part"][k][lo::stride]), k
        # the kept keys are the ids' strings, the ids their hashes
        assert all(isinstance(k, str) for k in r["keys"])
        assert np.array_equal(r["ids"], string_ref.keys([k.encode() for k in r["keys"]]))
        got = {k: tuple(v) for k, v in zip(r["keys"], r["vals"].tolist())}
        assert len(got) == len(r["keys"]) and got == dense["by_string"]
        assert [k for k, _ in r["iterated"]] == r["keys"]
        assert dict(r["iterated"]) == got
    assert 0 < len(dense["by_string"]) < N_PK  # private selection dropped some
    assert dense["part"]["count"].sum() < N  # the bounds bind
    # gather=True: the same keys and values on both ranks
    assert results[0]["keys"] == results[1]["keys"]
    assert np.array_equal(results[0]["vals"], results[1]["vals"])
    assert np.array_equal(results[0]["ids"], results[1]["ids"])


@pytest.mark.gpu
def test_two_ranks_public_partitions_equal_a_groupby(ranks):
    want = _groupby()
    for r in base._ok(ranks, "public"):
        got = {k: tuple(v) for k, v in zip(r["keys"], r["vals"].tolist())}
        assert len(r["keys"]) == N_PK + len(ABSENT) and got == want
        assert all(got[s] == (0.0, 0.0, 0.0) for s in ABSENT)
    assert sum(v[0] for v in want.values()) == N


@pytest.mark.gpu
def test_two_ranks_without_gather_hold_their_owned_partitions(ranks, rule, dense):
    ids, _ = rule
    results = base._ok(ranks, "owned")
    for rank, r in enumerate(results):
        assert all(ids[k] % WORLD == rank for k in r["keys"])
        got = {k: tuple(v) for k, v in zip(r["keys"], r["vals"].tolist())}
        assert got == {k: v for k, v in dense["by_string"].items() if ids[k] % WORLD == rank}
    a, b = set(results[0]["keys"]), set(results[1]["keys"])
    assert a and b and not (a & b)
    assert a | b == set(dense["by_string"])


@pytest.mark.gpu
def test_two_ranks_select_partitions(ranks, dense):
    """The selected strings are those of the one-process dense
    select_partitions of the ids under the same seed and nonce.  (Not the kept
    set of the aggregate release above: there the selection shares the budget
    with three metrics, so its thresholds differ.)"""
    print("selected:", len(dense["selected"]), "kept by the aggregate release:",
          len(dense["by_string"]), "equal:", dense["selected"] == sorted(dense["by_string"]))
    for r in base._ok(ranks, "select"):
        assert all(isinstance(k, str) for k in r)
        assert sorted(r) == dense["selected"] and 0 < len(r) < N_PK
    assert base._ok(ranks, "select")[0] == base._ok(ranks, "select")[1]


@pytest.mark.gpu
def test_two_ranks_shuffled_with_string_privacy_ids(ranks):
    want = _groupby()
    for r in base._ok(ranks, "shuffle"):
        got = {k: tuple(v) for k, v in zip(r["keys"], r["vals"].tolist())}
        assert len(r["keys"]) == N_PK + len(ABSENT) and got == want


@pytest.mark.gpu
def test_two_ranks_raise_together(ranks):
    want = ("ValueError", "1 records or strings share a 64-bit hash with a different string; "
                          "pass another hash_seed")
    assert [r["collision"] for r in ranks] == [want] * WORLD
    for r in ranks:
        assert r["bad_offsets"][0] == "ValueError", r["bad_offsets"]
        assert r["bad_offsets"][1].startswith("2 records of the partition key StringColumn")
    assert ranks[0]["bad_offsets"] == ranks[1]["bad_offsets"]


# ---------------------------------------------------------------- one process
@pytest.mark.gpu
def test_one_process_flagged_equals_unflagged_per_string(built):
    pid_s, pk_s, pid_i, pk_i, val = base._dataset()
    kw = dict(public=_public(), noise=False, binding=False)
    plain = _release(pid_i, base._column(pk_s), val, **kw)
    flagged = _release(pid_i, base._column(pk_s), val, global_string_keys=True, **kw)
    got = {k: tuple(v) for k, v in zip(flagged["keys"], flagged["vals"].tolist())}
    assert got == {k: tuple(v) for k, v in zip(plain["keys"], plain["vals"].tolist())}
    assert got == _groupby()
    # the ids are the ascending signed rank of the hashes, not of the strings
    ids, P = string_pack_ref.global_ids(_public(), 1)
    assert flagged["P"] == P == N_PK + len(ABSENT)
    assert np.array_equal(flagged["rec_ids"], np.array([ids[s] for s in pk_s]))
    by_hash = sorted(_public(), key=lambda s: int(string_ref.keys([s.encode()])[0]))
    assert [ids[s] for s in by_hash] == list(range(P))
    assert by_hash != sorted(_public())
    assert np.array_equal(flagged["ids"],
                          string_ref.keys([k.encode() for k in flagged["keys"]]))


@pytest.mark.gpu
def test_refusals_from_host_state(built):
    import pipelinedp_amd as pdp
    from pipelinedp_amd import analysis
    pid_s, pk_s, pid_i, pk_i, val = base._dataset()
    small = slice(0, 1000)
    ex = pdp.DataExtractors("pid", "pk", "value")

    def data(value):
        return pdp.ColumnarData(pid=base._cuda(pid_i[small]), pk=base._column(pk_s[small]),
                                value=base._cuda(value), global_string_keys=True)

    def aggregate(params, value, **backend):
        acc = pdp.NaiveBudgetAccountant(4.0, 1e-5)
        res = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=SEED, **backend)).aggregate(
            data(value), params, ex)
        acc.compute_budgets()
        return res.materialize()

    with pytest.raises(NotImplementedError, match="global_string_keys=True supports"):
        aggregate(base._params([pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50)]), val[small],
                  percentiles=True)
    with pytest.raises(NotImplementedError, match="global_string_keys=True supports"):
        aggregate(pdp.AggregateParams(
            metrics=[pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM], max_partitions_contributed=3,
            max_contributions_per_partition=2, vector_size=2, vector_max_norm=5.0,
            vector_norm_kind=pdp.NormKind.Linf, noise_kind=pdp.NoiseKind.GAUSSIAN),
            np.ones((1000, 2)), vector_sums=True)
    opts = analysis.UtilityAnalysisOptions(epsilon=1.0, delta=1e-6,
                                           aggregate_params=base._params([pdp.Metrics.COUNT]))
    with pytest.raises(NotImplementedError, match="global_string_keys=True is supported by"):
        reports, _ = analysis.perform_utility_analysis(
            data(val[small]), pdp.MI355XBackend(device=0, seed=SEED), opts, ex)
        list(reports)  # the analysis is lazy, like every release
