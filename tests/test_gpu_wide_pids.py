"""ColumnarData(wide_privacy_ids=True) through DPEngine, in one process and on
two ranks that share GPU 0 (gloo process group, as tests/test_gpu_sparse_keys.py).

200 000 records of 20 000 privacy ids drawn from [-2^62, 2^62) over 3 000
partitions; max_partitions_contributed=3 and max_contributions_per_partition=2
bind.  The values are integers: a partition's float sum is accumulated in an
order that is not fixed from run to run, and only sums of integers do not
depend on it, so every comparison of bounded releases is bit for bit.

One process: the flag gives the ids the default encoding gives (the ascending
rank of each id), so the releases are equal -- partials, kept set, noised
values.  Two ranks: each rank's ids are the ranks within its own id set, so the
release equals the "trusted" release in which every rank passes its locally
ranked narrow ids; where bounding drops nothing, rows and count equal the
one-process partials.

One pair of worker processes runs every two-rank release of this module, each
a release of its own; a release that raises is reported to the test that
checks it."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

SEED, NONCE = 0x1D5EED, 0x0DDBA11
WORLD = 2
N, N_PID, P = 200_000, 20_000, 3_000
I64_MIN = -(1 << 63)


def _dataset():
    rng = np.random.default_rng(2025)
    pool = np.unique(rng.integers(-(1 << 62), 1 << 62, N_PID + 100, dtype=np.int64))[:N_PID]
    rng.shuffle(pool)
    pid = pool[rng.integers(0, N_PID, N)]
    assert int(pid.max()) - int(pid.min()) >= 1 << 32
    pk = ((rng.zipf(1.1, N) - 1) % P).astype(np.int64)
    val = np.floor(rng.uniform(-1.0, 11.0, N))
    return pid, pk, val


def _n_distinct():
    return len(np.unique(_dataset()[0]))


def _split(shard_fn):
    """The dataset ordered shard by shard under shard_fn (rank r holds one
    contiguous block, its record ids are offset + i) and the blocks' starts."""
    pid, pk, val = _dataset()
    shard = shard_fn(torch.from_numpy(pid), WORLD).numpy()
    order = np.argsort(shard, kind="stable")
    starts = np.searchsorted(shard[order], np.arange(WORLD + 1))
    return pid[order], pk[order], val[order], starts


def _sparse(pk):
    """The partition ids as sparse int64 keys of either sign."""
    return pk * 1_000_003 - 1_500_000_001


def _params(binding=True):
    import pipelinedp_amd as pdp
    return pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        max_partitions_contributed=3 if binding else P,
        max_contributions_per_partition=2 if binding else N,
        min_value=0.0, max_value=10.0)


def _release(pid, pk, val, group, public=None, noise=True, binding=True, **cols):
    """One release; everything the tests compare, as numpy."""
    import pipelinedp_amd as pdp
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    data = pdp.ColumnarData(pid=torch.from_numpy(pid).cuda(), pk=torch.from_numpy(pk).cuda(),
                            value=torch.from_numpy(val).cuda(), **cols)
    res = pdp.DPEngine(acc, backend).aggregate(data, _params(binding),
                                               pdp.DataExtractors("pid", "pk", "value"),
                                               public_partitions=public)
    acc.compute_budgets()
    res.nonce = NONCE
    res.noise_enabled = noise
    out = res.materialize()
    part, lo, stride, n = res.last_slice
    return dict(lo=lo, stride=stride, n=n, pid_count=res.last_bound_fields["pid_count"],
                pid_min=res.last_bound_fields["pid_min"],
                part={k: v.cpu().numpy() for k, v in part.items() if v is not None},
                ids=out.partition_ids.cpu().numpy(), vals=out.values.cpu().numpy())


def _ranked(pid):
    """The narrow form of the same ids: their ascending ranks and the count."""
    uniq, inv = np.unique(pid, return_inverse=True)
    return inv.astype(np.int64), max(1, len(uniq))


def _assert_same_release(a, b):
    assert (a["lo"], a["stride"], a["n"]) == (b["lo"], b["stride"], b["n"])
    assert (a["pid_min"], a["pid_count"]) == (b["pid_min"], b["pid_count"])
    for k in ("rows", "count", "sum"):
        assert np.array_equal(a["part"][k], b["part"][k]), k
    assert np.array_equal(a["ids"], b["ids"])
    assert np.array_equal(a["vals"], b["vals"])


# ---------------------------------------------------------------- one process
@pytest.mark.gpu
def test_one_process_flag_equals_default_encoding(built):
    pid, pk, val = _dataset()
    flagged = _release(pid, pk, val, None, wide_privacy_ids=True)
    default = _release(pid, pk, val, None)
    _assert_same_release(flagged, default)
    assert flagged["pid_count"] == _n_distinct() > N_PID // 2 and 0 < len(flagged["ids"]) < P
    # bounding binds: fewer records are counted than there are
    assert flagged["part"]["count"].sum() < N
    # a table sized by the caller's bound gives the same release
    bounded = _release(pid, pk, val, None, wide_privacy_ids=True,
                       max_distinct_privacy_ids=N_PID)
    _assert_same_release(bounded, default)


@pytest.mark.gpu
def test_one_process_with_declared_partitions(built):
    """n_partitions=P skips the default encoding: wide ids without the flag are
    refused there, with it they release what their ranks release."""
    pid, pk, val = _dataset()
    narrow, D = _ranked(pid)
    flagged = _release(pid, pk, val, None, wide_privacy_ids=True, n_partitions=P)
    ranked = _release(narrow, pk, val, None, n_partitions=P, privacy_id_range=(0, D))
    _assert_same_release(flagged, ranked)
    with pytest.raises(ValueError, match="2\\^32"):
        _release(pid, pk, val, None, n_partitions=P)


@pytest.mark.gpu
def test_one_process_select_partitions(built):
    import pipelinedp_amd as pdp
    pid, pk, _ = _dataset()

    def select(**cols):
        backend = pdp.MI355XBackend(device=0, seed=SEED)
        acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
        data = pdp.ColumnarData(pid=torch.from_numpy(pid).cuda(), pk=torch.from_numpy(pk).cuda(),
                                **cols)
        sel = pdp.DPEngine(acc, backend).select_partitions(
            data, pdp.SelectPartitionsParams(max_partitions_contributed=3),
            pdp.DataExtractors("pid", "pk"))
        acc.compute_budgets()
        sel.nonce = NONCE
        return list(sel)

    got = select(wide_privacy_ids=True)
    assert got == select() and 0 < len(got) < P


@pytest.mark.gpu
def test_one_process_dataset_histograms(built):
    """An analysis entry point (pre_aggregation.device_pairs): the histograms
    of the wide ids are those of their ranks; every bin is an integer."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd.dataset_histograms import computing_histograms as ch
    from tests import hist_cases as hc
    pid, pk, val = _dataset()
    narrow, D = _ranked(pid)
    ex = pdp.DataExtractors("pid", "pk", "value")

    def hist(ids, **cols):
        backend = pdp.MI355XBackend(device=0, seed=SEED)
        col = pdp.ColumnarData(pid=torch.from_numpy(ids).cuda(), pk=torch.from_numpy(pk).cuda(),
                               value=torch.from_numpy(val).cuda(), n_partitions=P, **cols)
        (hs,) = list(ch.compute_dataset_histograms(col, ex, backend))
        return hc.plain(hs)

    got = hist(pid, wide_privacy_ids=True)
    assert got == hist(narrow, privacy_id_range=(0, D))
    l0 = dict(got)["l0_contributions"]
    assert sum(b[2] for b in l0) == D


@pytest.mark.gpu
def test_errors_in_one_process(built):
    pid, pk, val = _dataset()
    bad = pid.copy()
    bad[11] = I64_MIN
    with pytest.raises(ValueError, match="INT64_MIN"):
        _release(bad, pk, val, None, wide_privacy_ids=True)
    with pytest.raises(ValueError, match="max_distinct_privacy_ids=16"):
        _release(pid, pk, val, None, wide_privacy_ids=True, max_distinct_privacy_ids=16)


def test_construction_errors():
    import pipelinedp_amd as pdp
    pid, pk, val = _dataset()
    with pytest.raises(ValueError, match="privacy_id_range"):
        pdp.ColumnarData(pid=pid, pk=pk, value=val, wide_privacy_ids=True,
                         privacy_id_range=(0, 1 << 32))
    with pytest.raises(TypeError, match="needs integers"):
        pdp.ColumnarData(pid=pid.astype(np.float64), pk=pk, value=val, wide_privacy_ids=True)


# ------------------------------------------------------------------ two ranks
def _guarded(fn):
    try:
        return ("ok", fn())
    except Exception as e:  # reported to the parent, which asserts on it
        return (type(e).__name__, str(e))


def _worker(rank, port, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        g = dist.group.WORLD
        pid, pk, val, starts = _split(distributed.shard_of_wide)
        a, b = int(starts[rank]), int(starts[rank + 1])
        mine = (pid[a:b], pk[a:b], val[a:b])
        out = {}
        out["trusted"] = _guarded(lambda: _release(
            *mine, g, wide_privacy_ids=True, n_partitions=P, record_id_offset=a))
        narrow, D = _ranked(mine[0])
        out["ranked"] = _guarded(lambda: _release(
            narrow, mine[1], mine[2], g, n_partitions=P, record_id_offset=a,
            privacy_id_range=(0, D)))
        out["verify"] = _guarded(lambda: _release(
            *mine, g, wide_privacy_ids=True, n_partitions=P, record_id_offset=a,
            sharding="verify"))
        # the split a caller of the narrow shard function would have made
        o_pid, o_pk, o_val, o_starts = _split(distributed.shard_of)
        c, d = int(o_starts[rank]), int(o_starts[rank + 1])
        out["verify_old_split"] = _guarded(lambda: _release(
            o_pid[c:d], o_pk[c:d], o_val[c:d], g, wide_privacy_ids=True, n_partitions=P,
            record_id_offset=c, sharding="verify"))
        # round-robin: nearly every privacy id sits on both ranks
        r_pid, r_pk, r_val = _dataset()
        public = np.unique(_sparse(r_pk)).tolist()
        out["shuffle"] = _guarded(lambda: _release(
            r_pid[rank::WORLD], _sparse(r_pk[rank::WORLD]), r_val[rank::WORLD], g, public=public,
            noise=False, binding=False, wide_privacy_ids=True, sparse_partition_keys=True,
            sharding="shuffle"))
        # rank 1 holds no record
        e = len(pid) if rank == 0 else 0
        out["empty_rank"] = _guarded(lambda: _release(
            pid[:e], pk[:e], val[:e], g, wide_privacy_ids=True, n_partitions=P))
        bad = mine[0].copy()
        if rank == 0:
            bad[5] = I64_MIN  # on one rank only: every rank raises
        out["reserved"] = _guarded(lambda: _release(
            bad, mine[1], mine[2], g, wide_privacy_ids=True, n_partitions=P))
        out["too_small"] = _guarded(lambda: _release(
            *mine, g, wide_privacy_ids=True, n_partitions=P, max_distinct_privacy_ids=16))
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


@pytest.mark.gpu
def test_trusted_equals_locally_ranked_narrow_ids(ranks):
    from pipelinedp_amd import distributed
    wide, ranked = _ok(ranks, "trusted"), _ok(ranks, "ranked")
    pid, _, _, starts = _split(distributed.shard_of_wide)
    for rank, (w, r) in enumerate(zip(wide, ranked)):
        _assert_same_release(w, r)
        assert (w["lo"], w["stride"], w["n"]) == (rank, WORLD, P // WORLD)
        assert w["pid_count"] == len(np.unique(pid[starts[rank]:starts[rank + 1]]))
        assert 0 < len(w["ids"]) < P
    # both ranks hold a real share of the ids, and the gathered release
    assert min(w["pid_count"] for w in wide) > N_PID // 4
    assert sum(w["pid_count"] for w in wide) == _n_distinct()
    assert np.array_equal(wide[0]["ids"], wide[1]["ids"])
    assert np.array_equal(wide[0]["vals"], wide[1]["vals"])


@pytest.mark.gpu
def test_verify_passes_on_the_wide_split(ranks):
    for v, t in zip(_ok(ranks, "verify"), _ok(ranks, "trusted")):
        _assert_same_release(v, t)


def test_the_old_split_misplaces_records():
    """Runs without a GPU: a split by shard_of is not a split by shard_of_wide."""
    from pipelinedp_amd import distributed
    pid, _, _, starts = _split(distributed.shard_of)
    owner = distributed.shard_of_wide(torch.from_numpy(pid), WORLD).numpy()
    held_by = np.repeat(np.arange(WORLD), np.diff(starts))
    assert int((owner != held_by).sum()) > 0


@pytest.mark.gpu
def test_verify_refuses_the_old_split_on_both_ranks(ranks):
    from pipelinedp_amd import distributed
    pid, _, _, starts = _split(distributed.shard_of)
    owner = distributed.shard_of_wide(torch.from_numpy(pid), WORLD).numpy()
    n_bad = int((owner != np.repeat(np.arange(WORLD), np.diff(starts))).sum())
    for r in ranks:
        assert r["verify_old_split"][0] == "ValueError", r["verify_old_split"]
        assert f"{n_bad} records" in r["verify_old_split"][1]
        assert "shard_of_wide" in r["verify_old_split"][1]


@pytest.mark.gpu
def test_shuffled_round_robin_split_equals_one_process(ranks):
    """Non-binding bounds, noise off, every partition public: the released
    COUNT and PRIVACY_ID_COUNT are the one-process partials exactly, SUM to
    the summation-order tolerance of tests/test_gpu_shuffle_ranks.py."""
    results = _ok(ranks, "shuffle")
    pid, pk, val = _dataset()
    keys = _sparse(pk)
    public = np.unique(keys)
    one = _release(pid, keys, val, None, public=public.tolist(), noise=False, binding=False,
                   wide_privacy_ids=True, sparse_partition_keys=True)
    o1 = np.argsort(one["ids"])
    assert np.array_equal(one["ids"][o1], public)
    # nothing is dropped: every record is counted
    assert one["vals"][:, 0].sum() == N
    for r in results:
        o = np.argsort(r["ids"])
        assert np.array_equal(r["ids"][o], public)
        assert np.array_equal(r["vals"][o][:, 0], one["vals"][o1][:, 0])  # COUNT
        assert np.array_equal(r["vals"][o][:, 2], one["vals"][o1][:, 2])  # PRIVACY_ID_COUNT
        assert np.allclose(r["vals"][o][:, 1], one["vals"][o1][:, 1], rtol=1e-12, atol=1e-9)
    # each rank numbered the ids it received
    assert sum(r["pid_count"] for r in results) == _n_distinct()


@pytest.mark.gpu
def test_a_rank_without_records(ranks):
    """Rank 0 holds every record, so its ids are the one-process ids: each
    rank's owned slice is the one-process release's."""
    results = _ok(ranks, "empty_rank")
    from pipelinedp_amd import distributed
    pid, pk, val, _ = _split(distributed.shard_of_wide)
    one = _release(pid, pk, val, None, wide_privacy_ids=True, n_partitions=P)
    assert results[0]["pid_count"] == _n_distinct() and results[1]["pid_count"] == 1
    for rank, r in enumerate(results):
        own = np.arange(rank, P, WORLD)
        for k in ("rows", "count", "sum"):
            assert np.array_equal(r["part"][k], one["part"][k][own]), k
        assert np.array_equal(np.sort(r["ids"]), np.sort(one["ids"]))
    assert len(one["ids"]) > 0


@pytest.mark.gpu
def test_errors_on_two_ranks(ranks):
    for r in ranks:
        assert r["reserved"][0] == "ValueError" and "INT64_MIN" in r["reserved"][1]
        assert r["too_small"][0] == "ValueError"
        assert "max_distinct_privacy_ids=16" in r["too_small"][1]
    assert ranks[0]["reserved"] == ranks[1]["reserved"]
    assert ranks[0]["too_small"] == ranks[1]["too_small"]
