"""Utility analysis with several gloo ranks on GPU 0 (as
test_gpu_kept_ranks.py: RCCL refuses two ranks on one device) against the
oracle (oracle/utility_oracle.py) on the WHOLE dataset: every rank's reports,
the union of the ranks' per-partition results, each rank's keys (exactly its
owned partitions) and the integer RawStatistics.

The dataset: 60 000 records of 2000 privacy ids over 151 Zipf(1.1)
partitions, declared with n_partitions = 160 (ids 151..159 are absent), swept
over an 8 x 8 grid of (max_partitions_contributed,
max_contributions_per_partition) with SUM + COUNT + PRIVACY_ID_COUNT.  Every
owned slice has partitions on both sides of 100 pairs (the exact
Poisson-binomial and its normal approximation) and one above 1024 pairs (split
between accumulate runs).

One spawn per world size runs all of that world size's cases; the oracle runs
once per distinct (public partitions, sampling) and is shared."""
import functools
import os
import queue
import socket
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import utility_oracle as uo
from tests import ua_cases as uc

pytestmark = pytest.mark.gpu

SEED = 7
N, N_PID, P_DATA, P_ALL = 60_000, 2_000, 151, 160
EPS, DELTA = 1.0, 1e-6
METRICS = ["COUNT", "SUM", "PRIVACY_ID_COUNT"]
VALS = [2**i for i in range(8)]
MPC = [a for a in VALS for _ in VALS]
MCPP = [b for _ in VALS for b in VALS]
PUBLIC = list(range(0, P_ALL, 3))  # includes absent ids (153, 156, 159)
SAMPLING = 0.5


def _shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (pid.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _dataset():
    """pid, pk, value: shared and never written to."""
    rng = np.random.default_rng(31)
    pid = rng.integers(0, N_PID, N).astype(np.int64)
    w = np.arange(1, P_DATA + 1, dtype=np.float64) ** -1.1
    pk = rng.choice(P_DATA, size=N, p=w / w.sum()).astype(np.int64)
    return dict(pid=pid, pk=pk, value=rng.uniform(-1, 6, N))


def _split(data, world, rank, how):
    """Record indices of one rank."""
    n = len(data["pid"])
    if how == "sorted":  # the rank's block of the shard_of-sorted dataset
        return np.nonzero(_shard_np(data["pid"], world) == rank)[0]
    if how == "strided":
        return np.arange(rank, n, world)
    assert how == "rank0"  # rank 0 holds everything, the others nothing
    return np.arange(n) if rank == 0 else np.arange(0)


# case -> (split, sharding, public partitions, partitions_sampling_prob)
CASES2 = {
    "private_trusted": ("sorted", "trusted", False, 1),
    "private_shuffle": ("strided", "shuffle", False, 1),
    "verify_strided": ("strided", "verify", False, 1),
    "public": ("sorted", "trusted", True, 1),
    "sampling": ("sorted", "trusted", False, SAMPLING),
    "rank0_holds_all": ("rank0", "trusted", False, 1),
}
CASES3 = {k: CASES2[k] for k in ("private_trusted", "public")}
WORLDS = {2: CASES2, 3: CASES3}


def _analyze(data, case, idx, group):
    """One utility analysis over the records idx; plain-dict results."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd import analysis
    _, sharding, public, prob = case
    multi = analysis.MultiParameterConfiguration(
        max_partitions_contributed=MPC, max_contributions_per_partition=MCPP,
        min_sum_per_partition=[0.0] * 64, max_sum_per_partition=[float(b) for b in MCPP])
    params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE,
                                 metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM,
                                          pdp.Metrics.PRIVACY_ID_COUNT],
                                 max_partitions_contributed=1, max_contributions_per_partition=1,
                                 min_sum_per_partition=0.0, max_sum_per_partition=1.0)
    opts = analysis.UtilityAnalysisOptions(epsilon=EPS, delta=DELTA, aggregate_params=params,
                                           multi_param_configuration=multi,
                                           partitions_sampling_prob=prob)
    backend = pdp.MI355XBackend(device=0, seed=SEED, process_group=group)
    cols = pdp.ColumnarData(pid=torch.from_numpy(data["pid"][idx]).cuda(),
                            pk=torch.from_numpy(data["pk"][idx]).cuda(),
                            value=torch.from_numpy(data["value"][idx]).cuda(),
                            n_partitions=P_ALL, sharding=sharding)
    reports, per = analysis.perform_utility_analysis(
        cols, backend, opts, pdp.DataExtractors("pid", "pk", "value"),
        public_partitions=PUBLIC if public else None)
    reports = [uc.to_plain(r) for r in reports]
    return dict(reports=reports, per={k: uc.to_plain(v) for k, v in per},
                owned=per.analysis.owned)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        data = _dataset()
        for name, case in WORLDS[world].items():
            idx = _split(data, world, rank, case[0])
            try:
                q.put((rank, name, _analyze(data, case, idx, dist.group.WORLD)))
            except ValueError:
                q.put((rank, name, f"ValueError on rank {rank}:\n{traceback.format_exc()}"))
                # sharding='verify' raises on every rank after its collective:
                # the ranks still agree.  Any other ValueError ends the worker
                if case[1] != "verify":
                    break
            except (NotImplementedError, TypeError, AttributeError, KeyError, RuntimeError):
                q.put((rank, name, f"rank {rank}, {name}:\n{traceback.format_exc()}"))
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
        for name in WORLDS[world]:
            g.setdefault(name, f"rank {rank} ended with exit code {procs[rank].exitcode} "
                               f"before it finished {name}")
    return got


@pytest.fixture(scope="module")
def world2(built):
    return _run(2)


@pytest.fixture(scope="module")
def world3(built):
    return _run(3)


def _sampler():
    from pipelinedp_amd.analysis import utility_analysis as ua_mod
    bound = ua_mod._sample_bound(SAMPLING)
    return lambda k: ua_mod._keep_by_hash(k, bound)


@functools.lru_cache(maxsize=None)
def _oracle(public, prob):
    """(per-partition results, reports) of the oracle on the whole dataset."""
    data = _dataset()
    pub = PUBLIC if public else None
    cfgs = [dict(mpc=a, mcpp=b, min_sum=0.0, max_sum=float(b), noise_kind="LAPLACE",
                 strategy="TRUNCATED_GEOMETRIC", pre_threshold=None) for a, b in zip(MPC, MCPP)]
    pairs = uo.preaggregate(data["pid"].tolist(), data["pk"].tolist(), data["value"].tolist(), pub)
    return uo.analyze(pairs, cfgs, METRICS, EPS, DELTA, "LAPLACE", public=pub,
                      sampled=_sampler() if prob < 1 else None)


_ONE = {}


def _one_process(name):
    """The same analysis in one process over the whole dataset."""
    case = CASES2[name]
    key = case[2:]
    if key not in _ONE:
        data = _dataset()
        _ONE[key] = _analyze(data, ("", "trusted") + key, np.arange(N), None)
    return _ONE[key]


def _max_dev(want, got):
    """Largest |want - got| / max(1, |want|) over the numbers of nested results."""
    if isinstance(want, dict):
        return max([_max_dev(v, got[k]) for k, v in want.items()] + [0.0])
    if isinstance(want, list):
        return max([_max_dev(a, b) for a, b in zip(want, got)] + [0.0])
    if isinstance(want, bool) or want is None or isinstance(want, str):
        return 0.0
    return abs(float(want) - float(got)) / max(1.0, abs(float(want)))


def _check(ranks, name):
    world = len(ranks)
    case = CASES2[name]
    want_per, want_rep = _oracle(case[2], case[3])
    assert len(want_per) > 0
    keys = set()
    for rank, got in enumerate(ranks):
        got = got[name]
        assert not isinstance(got, str), got
        # every rank's reports are the whole dataset's
        assert len(got["reports"]) == len(want_rep) == 64
        for want, have in zip(want_rep, got["reports"]):
            uc.assert_close(want, have, f"rank {rank} report", atol=1e-7, rtol=1e-7)
        # each rank's keys are exactly its owned ones
        assert got["owned"] == (rank, world, len(range(rank, P_ALL, world)))
        mine = {k for k in want_per if k[0] % world == rank}
        assert set(got["per"]) == mine, (name, rank)
        assert not keys & set(got["per"])
        keys |= set(got["per"])
        for key in mine:
            want, have = want_per[key], got["per"][key]
            uc.assert_close(want, have, f"rank {rank} per{key}", atol=1e-7, rtol=1e-7)
            assert have["raw_statistics"] == want["raw_statistics"], key  # integers: exact
    assert keys == set(want_per)  # the union is the one-process key set
    one = _one_process(name)
    assert set(one["per"]) == keys
    dev = max(_max_dev(one["per"][k], g[name]["per"][k]) for g in ranks for k in g[name]["per"])
    dev_rep = max(_max_dev(one["reports"], g[name]["reports"]) for g in ranks)
    print(f"{name}, {world} ranks: largest deviation from the one-process run "
          f"per partition {dev:.3e}, reports {dev_rep:.3e}")
    for g in ranks:  # integer outputs: bit for bit against one process
        for k, v in g[name]["per"].items():
            assert v["raw_statistics"] == one["per"][k]["raw_statistics"]


def test_dataset_covers_both_regimes_on_every_rank():
    data = _dataset()
    pairs = np.unique(data["pid"] * P_ALL + data["pk"]) % P_ALL
    sizes = np.bincount(pairs, minlength=P_ALL)
    assert (sizes[P_DATA:] == 0).all() and len(data["pid"]) == N
    for world in (2, 3):
        for rank in range(world):
            s = sizes[rank::world]
            s = s[s > 0]
            assert (s < 100).any() and (s > 100).any() and (s > 1024).any(), (world, rank)
            # every rank holds records under every split that is meant to
            assert len(_split(data, world, rank, "sorted")) > 0


@pytest.mark.parametrize("name", ["private_trusted", "private_shuffle", "rank0_holds_all"])
def test_private_partitions(built, world2, name):
    _check(world2, name)


def test_verify_raises_on_every_rank(built, world2):
    for rank, got in enumerate(world2):
        got = got["verify_strided"]
        assert isinstance(got, str) and got.startswith("ValueError"), got
        assert "sharding='verify'" in got and "use sharding='shuffle'" in got
    # the ranks went on together: the cases after it ran
    assert not isinstance(world2[0]["public"], str), world2[0]["public"]


def test_public_partitions_with_absent_ids(built, world2):
    want_per, _ = _oracle(True, 1)
    assert {k[0] for k in want_per} == set(PUBLIC) and 159 in PUBLIC
    _check(world2, "public")


def test_partition_sampling(built, world2):
    want_per, _ = _oracle(False, SAMPLING)
    kept = {k[0] for k in want_per}
    assert 0 < len(kept) < P_DATA and len({k % 2 for k in kept}) == 2
    _check(world2, "sampling")


@pytest.mark.parametrize("name", ["private_trusted", "public"])
def test_three_ranks(built, world3, name):
    _check(world3, name)
