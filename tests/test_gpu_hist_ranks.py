"""Dataset histograms, private contribution bounds and tune with several gloo
ranks on GPU 0 (as test_gpu_utility_ranks.py: RCCL refuses two ranks on one
device) against the oracle (oracle/hist_oracle.py) on the WHOLE dataset, the
other ranks and the one-process GPU run.

The dataset (tests/hist_cases.py): 80 000 records of 2500 privacy ids over 1290
Zipf(1.1) partitions, n_partitions = 1301 declared (11 ids absent); values are
eighths, so every sum is exact in any order and the whole comparison, LINF_SUM
included, is bit for bit.  One privacy id has 1100 partitions and one pair has
1200 records (bins >= 1000: the global atomics); the smallest and the largest
pair sum sit on different ranks.  A second set of values, uniform(-1, 6), is
held to test_gpu_histograms.py::assert_same's rule.

One spawn per world size runs all of that world size's cases."""
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

from oracle import hist_oracle
from tests import hist_cases as hc
from tests import ua_cases as uc

pytestmark = pytest.mark.gpu

P = hc.P_ALL
PARTS = list(range(0, P, 2))
UPPER = 2000
REPEATS = 10

# case -> (kind, split, sharding)
CASES2 = {
    "trusted": ("hist", "sorted", "trusted"),
    "shuffle": ("hist", "strided", "shuffle"),
    "verify_sorted": ("hist", "sorted", "verify"),
    "verify_strided": ("hist", "strided", "verify"),
    "rank0_holds_all": ("hist", "rank0", "trusted"),
    "sparse_exchange": ("hist_sparse", "sorted", "trusted"),
    "uniform": ("hist_uniform", "sorted", "trusted"),
    "bounds": ("bounds", "sorted", "trusted"),
    "bounds_draws": ("bounds_draws", "sorted", "trusted"),
    "tune": ("tune", "sorted", "trusted"),
}
CASES3 = {k: CASES2[k] for k in ("trusted", "shuffle", "rank0_holds_all", "bounds", "tune")}
WORLDS = {2: CASES2, 3: CASES3}


def _bounds_params(eps):
    import pipelinedp_amd as pdp
    return pdp.CalculatePrivateContributionBoundsParams(
        aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=1.0, aggregation_delta=0.0,
        calculation_eps=eps, max_partitions_contributed_upper_bound=UPPER)


def _run_case(kind, data, idx, sharding, group):
    """One case over the records idx; plain results."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd.analysis import parameter_tuning as pt
    from pipelinedp_amd.dataset_histograms import computing_histograms as ch
    ex = pdp.DataExtractors("pid", "pk", "value")
    # 'auto' takes the dense exchange of the totals at this P; hist_sparse
    # forces the all-to-all of the occupied partitions' rows
    backend = pdp.MI355XBackend(device=0, seed=7, process_group=group,
                                exchange="all_to_all" if kind == "hist_sparse" else "auto")
    col = pdp.ColumnarData(pid=torch.from_numpy(data["pid"][idx]).cuda(),
                           pk=torch.from_numpy(data["pk"][idx]).cuda(),
                           value=torch.from_numpy(data["value"][idx]).cuda(),
                           n_partitions=P, sharding=sharding)
    if kind in ("hist", "hist_uniform", "hist_sparse"):
        (hs,) = list(ch.compute_dataset_histograms(col, ex, backend))
        return hc.plain(hs)
    if kind in ("bounds", "bounds_draws"):
        engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(1, 1e-6), backend)
        out = []
        for _ in range(1 if kind == "bounds" else REPEATS):
            (res,) = list(engine.calculate_private_contribution_bounds(
                col, _bounds_params(1e6 if kind == "bounds" else 1e-3), ex, PARTS))
            out.append(res.max_partitions_contributed)
        return out
    assert kind == "tune"
    (hs,) = list(ch.compute_dataset_histograms(col, ex, backend))
    params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                 max_partitions_contributed=1, max_contributions_per_partition=1)
    opts = pt.TuneOptions(epsilon=1.0, delta=1e-6, aggregate_params=params,
                          function_to_minimize=pt.MinimizingFunction.ABSOLUTE_ERROR,
                          parameters_to_tune=pt.ParametersToTune(True, True),
                          number_of_parameter_candidates=100)
    res_col, _ = pt.tune(col, backend, hs, opts, ex)
    (res,) = list(res_col)
    return dict(parameters=uc.to_plain(res.utility_analysis_parameters),
                index_best=res.index_best, reports=[uc.to_plain(r) for r in res.utility_reports])


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name, (kind, how, sharding) in WORLDS[world].items():
            data = hc.dataset(exact=kind != "hist_uniform")
            idx = hc.split(data, world, rank, how)
            try:
                q.put((rank, name, _run_case(kind, data, idx, sharding, dist.group.WORLD)))
            except ValueError:
                q.put((rank, name, f"ValueError on rank {rank}:\n{traceback.format_exc()}"))
                # sharding='verify' raises on every rank after its collective:
                # the ranks still agree.  Any other ValueError ends the worker
                if sharding != "verify":
                    break
            except (NotImplementedError, TypeError, AttributeError, KeyError, RuntimeError,
                    AssertionError):
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


@functools.lru_cache(maxsize=None)
def _oracle(exact=True):
    d = hc.dataset(exact)
    return hc.as_lists(hist_oracle.dataset_histograms(d["pid"], d["pk"], d["value"]))


_ONE = {}


def _one_process(kind):
    """The same call in one process over the whole dataset."""
    if kind not in _ONE:
        data = hc.dataset(exact=kind != "hist_uniform")
        _ONE[kind] = _run_case(kind, data, np.arange(hc.N), "trusted", None)
    return _ONE[kind]


def _results(ranks, name):
    for got in ranks:
        assert not isinstance(got[name], str), got[name]
    return [got[name] for got in ranks]


def test_dataset_preconditions():
    """What makes a sum of per-rank bins wrong is in the data: for both world
    sizes a partition with >= 1000 records (pairs) in total and fewer on every
    rank, partitions occupied on one rank only, the min and the max pair sum on
    different ranks, and a bin with lower >= 1000 in every histogram."""
    d = hc.dataset()
    pid, pk = d["pid"], d["pk"]
    assert len(pid) == hc.N and pk.max() == hc.P_DATA - 1 < P - 1
    pairs = np.unique(pid * P + pk)
    ppid, ppk = pairs // P, pairs % P
    rec, prs = np.bincount(pk, minlength=P), np.bincount(ppk, minlength=P)
    sums = np.zeros(len(pairs))
    np.add.at(sums, np.searchsorted(pairs, pid * P + pk), d["value"])
    for world in (2, 3):
        sh, shp = hc.shard_np(pid, world), hc.shard_np(ppid, world)
        rr = np.stack([np.bincount(pk[sh == r], minlength=P) for r in range(world)])
        pr = np.stack([np.bincount(ppk[shp == r], minlength=P) for r in range(world)])
        assert ((rec >= 1000) & (rr.max(0) < 1000)).any(), world
        assert ((prs >= 1000) & (pr.max(0) < 1000)).any(), world
        assert ((pr > 0).sum(0) == 1).any(), world
        assert shp[np.argmin(sums)] != shp[np.argmax(sums)], world
        assert (rr.sum(1) > 0).all()
    for name, bins in _oracle():
        assert bins[-1][0] >= 1000, name
    assert len(_oracle()[0][1]) and _oracle()[0][1][-1][4] == 1100  # L0 of the wide id


@pytest.mark.parametrize("name", ["trusted", "shuffle", "verify_sorted", "rank0_holds_all",
                                  "sparse_exchange"])
def test_two_ranks_equal_oracle_and_one_process(built, world2, name):
    want = _oracle()
    one = _one_process("hist")
    assert one == want  # eighths: bit for bit, LINF_SUM included
    for rank, got in enumerate(_results(world2, name)):
        assert got == want, (name, rank)


@pytest.mark.parametrize("name", ["trusted", "shuffle", "rank0_holds_all"])
def test_three_ranks_equal_oracle_and_one_process(built, world3, name):
    want = _oracle()
    assert _one_process("hist") == want
    for rank, got in enumerate(_results(world3, name)):
        assert got == want, (name, rank)


def test_verify_raises_on_every_rank(built, world2):
    for got in world2:
        got = got["verify_strided"]
        assert isinstance(got, str) and got.startswith("ValueError"), got
        assert "sharding='verify'" in got and "use sharding='shuffle'" in got
    # the ranks went on together: the cases after it ran
    assert not isinstance(world2[0]["rank0_holds_all"], str), world2[0]["rank0_holds_all"]


def test_uniform_values_to_rounding(built, world2):
    """Pair sums that are not exact: assert_same's rule against the oracle;
    integers, LINF_SUM counts exact; every rank identical."""
    want = _oracle(exact=False)
    one = _one_process("hist_uniform")
    hc.assert_same(one, want, "one process")
    res = _results(world2, "uniform")
    dev = 0.0
    for rank, got in enumerate(res):
        hc.assert_same(got, want, f"rank {rank}")
        hc.assert_same(got, one, f"rank {rank} against one process")
        for x, y in zip(got[3][1], one[3][1]):
            dev = max([dev] + [abs(a - b) / max(1.0, abs(b)) for a, b in zip(x, y)])
        for i in (0, 1, 2, 4, 5):
            assert got[i] == one[i]
    assert res[0][:3] == res[1][:3] and res[0][4:] == res[1][4:]
    # the all-reduce gives every rank the same bits
    assert res[0][3] == res[1][3]
    print(f"uniform, 2 ranks: largest LINF_SUM deviation from the one-process run {dev:.3e}")


def _scoring(eps):
    """(scoring function, candidates) from the oracle's L0 histogram of the
    restricted rows (test_private_contribution_bounds_end_to_end's recipe)."""
    from pipelinedp_amd import private_contribution_bounds as pcb
    from pipelinedp_amd.dataset_histograms import histograms as hist
    d = hc.dataset()
    keep = np.isin(d["pk"], PARTS)
    (_, l0_bins), *_ = hist_oracle.dataset_histograms(d["pid"][keep], d["pk"][keep],
                                                      d["value"][keep])
    l0 = hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS,
                        [hist.FrequencyBin(*b) for b in l0_bins])
    return (pcb.L0ScoringFunction(_bounds_params(eps), len(PARTS), l0),
            pcb.generate_possible_contribution_bounds(UPPER))


def _best_bound():
    sf, cands = _scoring(1e6)
    return cands[int(np.argmax(sf.scores(cands)))]


@pytest.mark.parametrize("world", [2, 3])
def test_private_contribution_bounds(built, world2, world3, world):
    best = _best_bound()
    for rank, got in enumerate(_results({2: world2, 3: world3}[world], "bounds")):
        assert got == [best], (world, rank)


def test_private_bound_is_rank_zeros_draw(built, world2):
    """calculation_eps = 1e-3: two ranks drawing for themselves agree in one
    repetition with probability sum(p^2), in all of them with its 10th power
    (computed here from the oracle's histogram: below 1e-6)."""
    from pipelinedp_amd import dp_computations as dpc
    sf, cands = _scoring(1e-3)
    p = dpc.ExponentialMechanism(sf)._calculate_probabilities(1e-3, cands)
    assert float((p ** 2).sum()) ** REPEATS < 1e-6
    a, b = _results(world2, "bounds_draws")
    print(f"bounds drawn with calculation_eps = 1e-3: {a}")
    assert len(a) == REPEATS and a == b and set(a) <= set(cands)


@pytest.mark.parametrize("world", [2, 3])
def test_tune(built, world2, world3, world):
    one = _one_process("tune")
    n = len(one["reports"])
    assert n > 64
    for rank, got in enumerate(_results({2: world2, 3: world3}[world], "tune")):
        assert got["parameters"] == one["parameters"], rank
        assert got["index_best"] == one["index_best"], rank
        assert len(got["reports"]) == n
        for want, have in zip(one["reports"], got["reports"]):
            uc.assert_close(want, have, f"rank {rank} report", atol=1e-7, rtol=1e-7)
