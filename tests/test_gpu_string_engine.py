"""StringColumn as `pk` and as `pid` through DPEngine, in one process and on two
ranks that share GPU 0 (gloo process group, as tests/test_gpu_wide_pids.py).

20 000 records, 300 distinct partition strings (some non-ASCII, one empty) and
2 000 distinct privacy-id strings.  The values are integers, so a partition's
sum does not depend on the order of its additions and every comparison of
releases under one backend seed and nonce is bit for bit.

A string `pk` must release exactly what the same strings passed as a list
release: the device dictionary gives the ids the host encoding gives.  A string
`pid` must release exactly what its hashes release as wide privacy ids."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import string_ref

SEED, NONCE = 0x57C0DE, 0x0DDBA11
WORLD = 2
N, N_PK, N_PID = 20_000, 300, 2_000


def _names():
    pks = [f"partition/{i:03d}" for i in range(N_PK)]
    pks[0] = ""
    pks[1], pks[2], pks[3], pks[4] = "é", "zürich", "€uro", "日本語"
    pks[5], pks[6] = "\U00010000 astral", "￿ last of the BMP"
    pks[7] = "a much longer partition key, well past one 64-byte line: " + "x" * 40
    pids = [f"user-{i * 7919 % 100_003:06d}@example.org" for i in range(N_PID)]
    pids[0], pids[1] = "", "ü"
    return pks, pids


def _dataset():
    """(pid strings, pk strings, pid index, pk index, values)."""
    rng = np.random.default_rng(1812)
    pks, pids = _names()
    pk_i = (rng.zipf(1.2, N) - 1) % N_PK
    pid_i = rng.integers(0, N_PID, N)
    val = np.floor(rng.uniform(-1.0, 11.0, N))
    return [pids[i] for i in pid_i], [pks[i] for i in pk_i], pid_i, pk_i, val


def _column(strings, **kw):
    import pipelinedp_amd as pdp
    c = pdp.StringColumn.from_strings(strings, **kw)
    return pdp.StringColumn(torch.from_numpy(c.offsets).cuda(), torch.from_numpy(c.data).cuda(),
                            hash_seed=c.hash_seed)


def _hashes(strings, seed=0):
    return string_ref.keys([s.encode("utf-8") for s in strings], seed)


def _params(metrics=None, binding=True):
    import pipelinedp_amd as pdp
    return pdp.AggregateParams(
        metrics=metrics or [pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        max_partitions_contributed=3 if binding else N_PK,
        max_contributions_per_partition=2 if binding else N,
        min_value=0.0, max_value=10.0)


def _cuda(x):
    return torch.from_numpy(np.asarray(x)).cuda() if isinstance(x, np.ndarray) else x


def _release(pid, pk, val, group=None, public=None, noise=True, params=None, percentiles=False,
             **cols):
    """One release; everything the tests compare."""
    import pipelinedp_amd as pdp
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group,
                                percentiles=percentiles)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    data = pdp.ColumnarData(pid=_cuda(pid), pk=_cuda(pk), value=_cuda(val), **cols)
    res = pdp.DPEngine(acc, backend).aggregate(data, params or _params(),
                                               pdp.DataExtractors("pid", "pk", "value"),
                                               public_partitions=public)
    acc.compute_budgets()
    res.nonce = NONCE
    res.noise_enabled = noise
    try:
        out = res.materialize()
    except Exception:
        assert res.last_bound_fields is None, "raised after bounding had been set up"
        raise
    part = res.last_slice[0]
    return dict(pid_count=res.last_bound_fields["pid_count"],
                part={k: v.cpu().numpy() for k, v in part.items() if v is not None},
                keys=out.keys(), ids=out.partition_ids.cpu().numpy(),
                vals=out.values.cpu().numpy())


def _assert_same_release(a, b):
    assert a["pid_count"] == b["pid_count"]
    assert set(a["part"]) == set(b["part"]) >= {"rows", "count"}
    for k in a["part"]:  # MEAN keeps normalised sums, SUM the sum
        assert np.array_equal(a["part"][k], b["part"][k]), k
    assert a["keys"] == b["keys"]
    assert np.array_equal(a["ids"], b["ids"])
    assert np.array_equal(a["vals"], b["vals"])


@pytest.fixture(scope="module")
def listed(built):
    """The release of the strings passed as lists of str for `pk` (integer
    pid): what every string-pk release is compared with."""
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    return _release(pid_i, pk_s, val)


# ------------------------------------------------------------- pk as strings
@pytest.mark.gpu
def test_string_pk_equals_list_of_str(listed):
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    got = _release(pid_i, _column(pk_s), val)
    _assert_same_release(got, listed)
    assert all(isinstance(k, str) for k in got["keys"])
    assert 0 < len(got["keys"]) < N_PK  # private selection dropped some
    assert got["part"]["count"].sum() < N  # the bounds bind
    # a table sized by the caller's bound, another seed, int32 offsets: the same
    bounded = _release(pid_i, _column(pk_s, hash_seed=77), val, max_distinct_partition_keys=N_PK)
    _assert_same_release(bounded, listed)
    import pipelinedp_amd as pdp
    c = pdp.StringColumn.from_strings(pk_s)
    narrow = pdp.StringColumn(torch.from_numpy(c.offsets.astype(np.int32)), c.data)  # host, int32
    _assert_same_release(_release(pid_i, narrow, val), listed)


@pytest.mark.gpu
def test_string_pk_mean_with_public_strings(built):
    import pipelinedp_amd as pdp
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    pks, _ = _names()
    public = pks[:40] + ["absent from the data Ω"]
    params = _params([pdp.Metrics.MEAN])
    want = _release(pid_i, pk_s, val, public=public, params=params)
    got = _release(pid_i, _column(pk_s), val, public=public, params=params)
    _assert_same_release(got, want)
    assert sorted(got["keys"]) == sorted(public)
    # the public partitions as a StringColumn
    again = _release(pid_i, _column(pk_s), val, public=_column(public), params=params)
    _assert_same_release(again, want)
    with pytest.raises(TypeError, match="list or tuple of str"):
        _release(pid_i, _column(pk_s), val, public=[1, 2], params=params)


@pytest.mark.gpu
def test_string_pk_select_partitions(built):
    import pipelinedp_amd as pdp
    pid_s, pk_s, pid_i, pk_i, val = _dataset()

    def select(pid, pk):
        backend = pdp.MI355XBackend(device=0, seed=SEED)
        acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
        sel = pdp.DPEngine(acc, backend).select_partitions(
            pdp.ColumnarData(pid=_cuda(pid), pk=pk),
            pdp.SelectPartitionsParams(max_partitions_contributed=3),
            pdp.DataExtractors("pid", "pk"))
        acc.compute_budgets()
        sel.nonce = NONCE
        return list(sel)

    got = select(pid_i, _column(pk_s))
    assert got == select(pid_i, pk_s) and 0 < len(got) < N_PK
    assert select(_column(pid_s), _column(pk_s)) == select(_hashes(pid_s), pk_s) != []


@pytest.mark.gpu
def test_string_pk_percentile(built):
    import pipelinedp_amd as pdp
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    rng = np.random.default_rng(3)
    val = rng.uniform(-1.0, 11.0, N)
    params = _params([pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50)])
    want = _release(pid_i, pk_s, val, params=params, percentiles=True)
    got = _release(pid_i, _column(pk_s), val, params=params, percentiles=True)
    assert got["keys"] == want["keys"] and len(got["keys"]) > 0
    assert np.array_equal(got["vals"], want["vals"])


# ------------------------------------------------------------ pid as strings
@pytest.mark.gpu
def test_string_pid_equals_its_hashes_as_wide_ids(built):
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    got = _release(_column(pid_s), pk_i, val)
    want = _release(_hashes(pid_s), pk_i, val, wide_privacy_ids=True)
    _assert_same_release(got, want)
    assert got["pid_count"] == N_PID and got["part"]["count"].sum() < N  # binding
    seeded = _release(_column(pid_s, hash_seed=5), pk_i, val, max_distinct_privacy_ids=N_PID)
    _assert_same_release(seeded, _release(_hashes(pid_s, 5), pk_i, val, wide_privacy_ids=True))


@pytest.mark.gpu
def test_string_pid_equals_list_of_str_where_nothing_is_bounded(built):
    """The ids differ (ranks of the hashes, ranks of the strings), so the
    samplers would differ; with bounds that do not bind nothing is sampled."""
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    got = _release(_column(pid_s), pk_i, val, params=_params(binding=False))
    want = _release(pid_s, pk_i, val, params=_params(binding=False))
    _assert_same_release(got, want)
    assert got["part"]["count"].sum() == N


@pytest.mark.gpu
def test_both_columns_as_strings(listed):
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    got = _release(_column(pid_s), _column(pk_s), val)
    want = _release(_hashes(pid_s), pk_s, val, wide_privacy_ids=True)
    _assert_same_release(got, want)
    assert got["keys"] != [] and set(got["keys"]) <= set(_names()[0])


# -------------------------------------------------------------------- errors
@pytest.mark.gpu
def test_a_hash_collision_raises(built, monkeypatch):
    """Hashes cut to two bits: 300 strings share four slots, and every record
    that is not its slot's first string is a mismatch."""
    from pipelinedp_amd import string_columns
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    real = string_columns.device_keys

    def two_bits(*args, **kw):
        keys, info = real(*args, **kw)
        return keys & 3, info

    monkeypatch.setattr(string_columns, "device_keys", two_bits)
    h = _hashes(pk_s) & 3
    first = {int(s): pk_s[int(np.nonzero(h == s)[0][0])] for s in np.unique(h)}
    mismatches = sum(1 for s, k in zip(h.tolist(), pk_s) if first[s] != k)
    assert 0 < mismatches < N
    with pytest.raises(ValueError, match=f"^{mismatches} records share a 64-bit hash with a "
                                         f"different string; pass another hash_seed"):
        _release(pid_i, _column(pk_s), val)


@pytest.mark.gpu
def test_errors(built):
    import pipelinedp_amd as pdp
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    col = _column(pk_s)
    bad = col.offsets.clone()
    bad[10] = bad[11] + 1     # record 9 runs past record 10's end; record 10: end < start
    bad[-1] += 1              # the last record ends past the data
    with pytest.raises(ValueError, match="^2 records of the partition key StringColumn"):
        _release(pid_i, pdp.StringColumn(bad, col.data), val)
    pcol = _column(pid_s)
    bad = pcol.offsets.clone()
    bad[0] = -1
    with pytest.raises(ValueError, match="^1 records of the privacy id StringColumn"):
        _release(pdp.StringColumn(bad, pcol.data), pk_i, val)
    with pytest.raises(ValueError, match="max_distinct_partition_keys=16"):
        _release(pid_i, col, val, max_distinct_partition_keys=16)
    with pytest.raises(ValueError, match="n_partitions must not be given"):
        _release(pid_i, col, val, n_partitions=N_PK)
    with pytest.raises(ValueError, match="privacy_id_range must not be given"):
        _release(pcol, pk_i, val, privacy_id_range=(0, N_PID))


@pytest.mark.gpu
def test_device_hash_of_a_column(built):
    from pipelinedp_amd import distributed
    pid_s = _dataset()[0][:500]
    got = distributed.string_key_hash(_column(pid_s, hash_seed=3))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), _hashes(pid_s, 3))


# ------------------------------------------------------------------ two ranks
def _guarded(fn):
    try:
        return ("ok", fn())
    except Exception as e:  # reported to the parent, which asserts on it
        return (type(e).__name__, str(e))


def _wide_split():
    """The dataset ordered shard by shard under shard_of_wide of the string
    hashes, and the blocks' starts."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd import distributed
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    keys = distributed.string_key_hash(pdp.StringColumn.from_strings(pid_s))
    shard = distributed.shard_of_wide(keys, WORLD).numpy()
    order = np.argsort(shard, kind="stable")
    starts = np.searchsorted(shard[order], np.arange(WORLD + 1))
    return [pid_s[i] for i in order], pk_i[order], val[order], starts


def _worker(rank, port, q):
    import pipelinedp_amd as pdp
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        g = dist.group.WORLD
        pid_s, pk_i, val, starts = _wide_split()
        a, b = int(starts[rank]), int(starts[rank + 1])
        out = {}
        out["trusted"] = _guarded(lambda: _release(
            _column(pid_s[a:b]), pk_i[a:b], val[a:b], g, n_partitions=N_PK, record_id_offset=a))
        out["verify"] = _guarded(lambda: _release(
            _column(pid_s[a:b]), pk_i[a:b], val[a:b], g, n_partitions=N_PK, record_id_offset=a,
            sharding="verify"))
        # round-robin: nearly every privacy id sits on both ranks
        r_pid, r_pk, _, r_pki, r_val = _dataset()
        out["shuffle"] = _guarded(lambda: _release(
            _column(r_pid[rank::WORLD]), r_pki[rank::WORLD], r_val[rank::WORLD], g,
            public=list(range(N_PK)), noise=False, params=_params(binding=False),
            n_partitions=N_PK, sharding="shuffle"))
        out["string_pk"] = _guarded(lambda: _release(
            r_pki[rank::WORLD], _column(r_pk[rank::WORLD]), r_val[rank::WORLD], g))
        col = _column(pid_s[a:b])
        if rank == 0:
            col.offsets[3] = -1  # on one rank only: every rank raises
        out["bad_offsets"] = _guarded(lambda: _release(
            col, pk_i[a:b], val[a:b], g, n_partitions=N_PK, record_id_offset=a))
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
def test_two_ranks_verify_passes_on_the_hash_split(ranks):
    pid_s, _, _, starts = _wide_split()
    for rank, (v, t) in enumerate(zip(_ok(ranks, "verify"), _ok(ranks, "trusted"))):
        _assert_same_release(v, t)
        assert v["pid_count"] == len(set(pid_s[starts[rank]:starts[rank + 1]])) > N_PID // 4
    assert sum(t["pid_count"] for t in _ok(ranks, "trusted")) == N_PID


@pytest.mark.gpu
def test_two_ranks_shuffled_round_robin_split_equals_one_process(ranks):
    """Non-binding bounds, noise off, every partition public: COUNT and
    PRIVACY_ID_COUNT are the one-process release exactly, SUM to the
    summation-order tolerance of tests/test_gpu_wide_pids.py (the values are
    integers, so it is exact here too)."""
    results = _ok(ranks, "shuffle")
    pid_s, pk_s, pid_i, pk_i, val = _dataset()
    one = _release(_column(pid_s), pk_i, val, public=list(range(N_PK)), noise=False,
                   params=_params(binding=False), n_partitions=N_PK)
    o1 = np.argsort(one["ids"])
    assert np.array_equal(one["ids"][o1], np.arange(N_PK))
    assert one["vals"][:, 0].sum() == N
    for r in results:
        o = np.argsort(r["ids"])
        assert np.array_equal(r["ids"][o], np.arange(N_PK))
        assert np.array_equal(r["vals"][o][:, 0], one["vals"][o1][:, 0])  # COUNT
        assert np.array_equal(r["vals"][o][:, 2], one["vals"][o1][:, 2])  # PRIVACY_ID_COUNT
        assert np.allclose(r["vals"][o][:, 1], one["vals"][o1][:, 1], rtol=1e-12, atol=1e-9)
    assert sum(r["pid_count"] for r in results) == N_PID


@pytest.mark.gpu
def test_two_ranks_refuse_a_string_pk(ranks):
    for r in ranks:
        assert r["string_pk"][0] == "NotImplementedError", r["string_pk"]
        assert "one process" in r["string_pk"][1]
    assert ranks[0]["string_pk"] == ranks[1]["string_pk"]


@pytest.mark.gpu
def test_two_ranks_raise_together_for_invalid_offsets(ranks):
    for r in ranks:
        assert r["bad_offsets"][0] == "ValueError", r["bad_offsets"]
        assert r["bad_offsets"][1].startswith("2 records of the privacy id StringColumn")
    assert ranks[0]["bad_offsets"] == ranks[1]["bad_offsets"]
