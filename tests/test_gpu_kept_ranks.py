"""PERCENTILE and VECTOR_SUM releases with several gloo ranks on GPU 0 (as
test_gpu_shuffle_ranks.py: RCCL refuses two ranks on one device), against the
one-process release of the whole dataset under the same seed and nonce.

The dataset never samples records: every privacy id has 6 distinct
partitions (max_partitions_contributed = 3 binds) and every (privacy id,
partition) pair one or two records (max_contributions_per_partition = 2
never binds), so the kept records are the same however the records are
placed, and a multi-rank release can be compared with the one-process one:

* percentiles, noise included: bit for bit;
* VECTOR_SUM of integer-valued rows, Gaussian noise included: bit for bit;
  each rank's merged sums are the one-process sums of its slice;
* VECTOR_SUM of float rows: to 1e-12 x sum |v| (tests/test_gpu_vector_sum.py's
  summation-order bound), and two multi-rank runs agree bit for bit.

One spawn per world size runs all of that world size's cases."""
import functools
import os
import queue
import socket
import sys
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import vector_ref

pytestmark = pytest.mark.gpu

SEED, NONCE = 0xAB5EED, 0x1234ABCD
N_PID, D = 4_000, 5
LO, HI = 0.0, 64.0
MAX_NORM = 100.0  # L2: a partition of one kept row is below it, the hot partitions far above
BIG = 1e9


def _shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (pid.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _dataset(P):
    """pid, pk and three value columns (scalars, integer rows, float rows),
    shared and never written to.  Partition P - 1 is absent from the data."""
    rng = np.random.default_rng(12 + P)
    draws = (rng.zipf(1.1, (N_PID, 64)) - 1) % (P - 1)
    pair_pid, pair_pk = [], []
    for p in range(N_PID):
        _, first = np.unique(draws[p], return_index=True)
        assert len(first) >= 6
        pair_pk.append(draws[p][np.sort(first)[:6]])
        pair_pid.append(np.full(6, p))
    pair_pid, pair_pk = np.concatenate(pair_pid), np.concatenate(pair_pk)
    reps = rng.integers(1, 3, len(pair_pid))
    pid, pk = np.repeat(pair_pid, reps), np.repeat(pair_pk, reps)
    o = rng.permutation(len(pid))
    pid, pk = pid[o].astype(np.int64), pk[o].astype(np.int64)
    n = len(pid)
    return dict(pid=pid, pk=pk, scalar=rng.uniform(LO - 4.0, HI + 4.0, n),
                ints=rng.integers(-3, 14, (n, D)).astype(np.float64),
                floats=rng.uniform(-1.0, 1.0, (n, D)))


def _split(data, world, rank, how):
    """(record indices, record id offset) of one rank."""
    n = len(data["pid"])
    if how == "sorted":  # the rank's block of the shard_of-sorted dataset
        shard = _shard_np(data["pid"], world)
        order = np.argsort(shard, kind="stable")
        starts = np.searchsorted(shard[order], np.arange(world + 1))
        return order[starts[rank]:starts[rank + 1]], int(starts[rank])
    if how == "strided":
        return np.arange(rank, n, world), 0
    assert how == "rank0"  # rank 0 holds everything, the others nothing
    return (np.arange(n) if rank == 0 else np.arange(0)), 0


# case -> (metric kind, value column, split, sharding, public partitions, noise)
CASES2 = {
    "pct_public": ("pct", "scalar", "sorted", "trusted", "half", True),
    "pct_private": ("pct", "scalar", "sorted", "trusted", None, True),
    "pct_shuffle": ("pct", "scalar", "strided", "shuffle", None, True),
    "vec_trusted": ("vec", "ints", "sorted", "trusted", "all", True),
    "vec_shuffle": ("vec", "ints", "strided", "shuffle", None, True),
    "vec_float": ("vecf", "floats", "sorted", "trusted", "all", False),
    "vec_float_again": ("vecf", "floats", "sorted", "trusted", "all", False),
    "pct_empty_rank": ("pct", "scalar", "rank0", "trusted", None, True),
    "vec_empty_rank": ("vec", "ints", "rank0", "trusted", "all", True),
}
CASES3 = {k: CASES2[k] for k in ("pct_public", "vec_trusted")}
WORLDS = {2: (3001, CASES2), 3: (1000, CASES3)}


def _public(which, P):
    if which is None:
        return None
    # "half": every second id and P - 1, which is absent from the data
    return sorted(set(range(0, P, 2)) | {P - 1}) if which == "half" else list(range(P))


def _release(data, P, case, idx, offset, group):
    import pipelinedp_amd as pdp
    kind, column, _, sharding, public, noise = case
    if kind == "pct":
        params = pdp.AggregateParams(
            metrics=[pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50), pdp.Metrics.PERCENTILE(90)],
            max_partitions_contributed=3, max_contributions_per_partition=2,
            min_value=LO, max_value=HI, noise_kind=pdp.NoiseKind.LAPLACE)
    else:
        l2 = kind == "vec"
        params = pdp.AggregateParams(
            metrics=[pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM],
            max_partitions_contributed=3, max_contributions_per_partition=2,
            vector_size=D, vector_max_norm=MAX_NORM if l2 else BIG,
            vector_norm_kind=pdp.NormKind.L2 if l2 else pdp.NormKind.Linf,
            noise_kind=pdp.NoiseKind.GAUSSIAN)
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group,
                                percentiles=kind == "pct", vector_sums=kind != "pct")
    acc = pdp.NaiveBudgetAccountant(4.0, 1e-5)
    cols = pdp.ColumnarData(pid=torch.from_numpy(data["pid"][idx]).cuda(),
                            pk=torch.from_numpy(data["pk"][idx]).cuda(),
                            value=torch.from_numpy(data[column][idx]).cuda(), n_partitions=P,
                            record_id_offset=int(offset), sharding=sharding)
    res = pdp.DPEngine(acc, backend).aggregate(cols, params,
                                               pdp.DataExtractors("pid", "pk", "value"),
                                               public_partitions=_public(public, P))
    acc.compute_budgets()
    res.noise_enabled = noise
    res.nonce = NONCE
    out = res.materialize()
    ids = out.partition_ids.cpu().numpy()
    o = np.argsort(ids, kind="stable")
    got = dict(ids=ids[o], values=out.values.cpu().numpy()[o], slice=res.last_slice[1:])
    if kind != "pct":
        got["sums"] = res.last_vector_sums.cpu().numpy()
    if group is None:
        got["keep"] = res.last_record_keep.cpu().numpy()
    return got


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P, cases = WORLDS[world]
        data = _dataset(P)
        for name, case in cases.items():
            idx, offset = _split(data, world, rank, case[2])
            try:
                q.put((rank, name, _release(data, P, case, idx, offset, dist.group.WORLD)))
            except (NotImplementedError, ValueError, TypeError, AttributeError, KeyError):
                # a host-side error, reported by the case's test; the ranks
                # may no longer agree on the next collective, so the later
                # cases do not run (a device error ends the worker at once)
                q.put((rank, name, f"rank {rank}, {name}:\n{traceback.format_exc()}"))
                if not isinstance(sys.exc_info()[1], NotImplementedError):
                    break
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world):
    """One spawn of `world` ranks; per rank, case -> result (or the traceback
    of a host-side error, or the exit code of a rank that ended before the
    case).  Returns as soon as every rank has ended."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [{} for _ in range(world)]
    deadline = time.monotonic() + 150
    try:
        while time.monotonic() < deadline:
            try:
                rank, name, res = q.get(timeout=0.5)
                got[rank][name] = res
            except queue.Empty:
                if not any(p.is_alive() for p in procs):
                    break
    finally:
        for p in procs:
            p.join(timeout=5)
            if p.is_alive():
                p.kill()
                p.join()
    for rank, g in enumerate(got):
        for name in WORLDS[world][1]:
            g.setdefault(name, f"rank {rank} ended with exit code {procs[rank].exitcode} "
                               f"before it finished {name}")
    return got


@pytest.fixture(scope="module")
def world2(built):
    return _run(2)


@pytest.fixture(scope="module")
def world3(built):
    return _run(3)


_ONE = {}


def _one_rank(P, name):
    """The one-process release of the whole dataset for a case's metrics,
    public partitions and noise (computed once per distinct release)."""
    case = WORLDS[2][1][name]
    key = (P, case[0], case[4], case[5])
    if key not in _ONE:
        data = _dataset(P)
        _ONE[key] = _release(data, P, case, np.arange(len(data["pid"])), 0, None)
    return _ONE[key]


def _assert_equal(ranks, want, name):
    for rank, got in enumerate(ranks):
        got = got[name]
        assert not isinstance(got, str), got
        assert np.array_equal(got["ids"], want["ids"]), (name, rank)
        assert got["values"].tobytes() == want["values"].tobytes(), (name, rank)


def _assert_slices(ranks, want, name, P):
    world = len(ranks)
    for rank, got in enumerate(ranks):
        lo, stride, n = got[name]["slice"]
        assert (lo, stride, n) == (rank, world, len(range(rank, P, world)))
        assert got[name]["sums"].tobytes() == want["sums"][rank::world].tobytes(), (name, rank)


def test_dataset_never_samples_records():
    for P in (3001, 1000):
        data = _dataset(P)
        pid, pk = data["pid"], data["pk"]
        pairs, per_pair = np.unique(pid * P + pk, return_counts=True)
        assert per_pair.max() == 2 and per_pair.min() == 1
        assert (np.bincount(pairs // P, minlength=N_PID) == 6).all()
        assert pk.max() < P - 1


def test_percentiles_public(built, world2):
    want = _one_rank(3001, "pct_public")
    assert want["ids"].tolist() == _public("half", 3001) and 3000 in want["ids"]
    assert want["values"].shape == (1501, 3)
    assert [g["pct_public"]["slice"][2] for g in world2] == [1501, 1500]
    _assert_equal(world2, want, "pct_public")


def test_percentiles_private(built, world2):
    want = _one_rank(3001, "pct_private")
    occupied = len(np.unique(_dataset(3001)["pk"]))
    assert 0 < len(want["ids"]) < occupied
    assert len(set(want["ids"] % 2)) == 2  # both ranks own kept partitions
    _assert_equal(world2, want, "pct_private")


def test_percentiles_shuffle(built, world2):
    _assert_equal(world2, _one_rank(3001, "pct_shuffle"), "pct_shuffle")


@pytest.mark.parametrize("name", ["vec_trusted", "vec_shuffle"])
def test_vector_integer_rows(built, world2, name):
    want = _one_rank(3001, name)
    norms = np.sqrt((want["sums"] ** 2).sum(1))[want["ids"]]
    assert (norms > MAX_NORM).any()  # the clip binds on some released partitions
    if name == "vec_trusted":
        assert ((norms > 0) & (norms <= MAX_NORM)).any() and len(want["ids"]) == 3001
    assert want["values"].shape[1] == 1 + D
    _assert_equal(world2, want, name)
    _assert_slices(world2, want, name, 3001)


def test_vector_float_rows(built, world2):
    want = _one_rank(3001, "vec_float")
    data = _dataset(3001)
    bound = 1e-12 * vector_ref.partition_sums(data["pk"], np.abs(data["floats"]), want["keep"],
                                              3001)  # summation order only
    assert want["ids"].tolist() == list(range(3001))
    for rank, got in enumerate(world2):
        a, b = got["vec_float"], got["vec_float_again"]
        assert not isinstance(a, str), a
        assert np.array_equal(a["ids"], want["ids"])
        assert a["values"].tobytes() == b["values"].tobytes()
        assert a["values"][:, 0].tobytes() == want["values"][:, 0].tobytes()  # count
        err = np.abs(a["values"][:, 1:] - want["values"][:, 1:])
        print(rank, (err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all()
    assert np.abs(want["values"][:, 1:]).sum() > 0


@pytest.mark.parametrize("name", ["pct_empty_rank", "vec_empty_rank"])
def test_one_rank_holds_no_records(built, world2, name):
    want = _one_rank(3001, name)
    assert len(want["ids"]) > 0
    _assert_equal(world2, want, name)
    if name == "vec_empty_rank":
        _assert_slices(world2, want, name, 3001)


def test_three_ranks_percentiles(built, world3):
    want = _one_rank(1000, "pct_public")
    assert want["ids"].tolist() == _public("half", 1000) and 999 in want["ids"]
    assert [g["pct_public"]["slice"][2] for g in world3] == [334, 333, 333]
    _assert_equal(world3, want, "pct_public")


def test_three_ranks_vector(built, world3):
    want = _one_rank(1000, "vec_trusted")
    _assert_equal(world3, want, "vec_trusted")
    _assert_slices(world3, want, "vec_trusted", 1000)
