"""distributed.exchange_owner_pairs on host tensors over gloo (world 2, 3 and
4) against a numpy model: all ranks' pk-sorted pairs concatenated in rank
order, a stable argsort by pk, and for every owner the entries with pk % R ==
rank re-based to pk // R with searchsorted starts.  P = 53 is divisible by no
world size, the last rank holds nothing and still takes part in every
collective.  Also: the calls that stay one-process raise NotImplementedError
under a 2-rank backend, before any device work (none of this needs a GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

N, P = 1501, 53


def _dataset():
    """Structured pair entries of the whole dataset, unsorted."""
    from pipelinedp_amd import pre_aggregation as pa
    rng = np.random.default_rng(21)
    a = np.zeros(N, dtype=pa.PAIR_DTYPE)
    a["pk"] = rng.integers(0, P, N)
    a["count"] = rng.integers(1, 9, N)
    a["sum"] = rng.uniform(-3.0, 3.0, N)
    a["np"] = rng.integers(1, 20, N)
    a["ncl"] = rng.integers(1, 50, N).astype(np.uint32) | (
        (rng.integers(0, 4, N) == 0).astype(np.uint32) << np.uint32(31))
    return a


def _local(world, rank):
    """One rank's pre-aggregate: its share of the pairs, ascending by pk."""
    a = _dataset()
    if rank == world - 1:
        return a[:0]
    mine = a[rank::world - 1]
    return mine[np.argsort(mine["pk"], kind="stable")]


def _words(a):
    return np.ascontiguousarray(a).view(np.float64).reshape(-1, 3)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mine = _local(world, rank)
        # a buffer longer than the count: the tail is not sent
        buf = torch.cat([torch.from_numpy(_words(mine).copy()),
                         torch.full((4, 3), 7.0, dtype=torch.float64)])
        pairs, starts, n_local, n, n_bad = distributed.exchange_owner_pairs(
            buf, len(mine), P, dist.group.WORLD)
        q.put((rank, pairs.numpy(), starts.numpy(), n_local, n, int(n_bad.item())))
    finally:
        dist.destroy_process_group()


def _guard_worker(rank, world, port, q):
    import torch.distributed as dist
    import pipelinedp_amd as pdp
    from pipelinedp_amd import analysis
    from pipelinedp_amd.analysis import parameter_tuning
    from pipelinedp_amd.dataset_histograms import computing_histograms
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        backend = pdp.MI355XBackend(device=0, seed=1, process_group=dist.group.WORLD)
        params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                     max_partitions_contributed=1,
                                     max_contributions_per_partition=1)
        rows = [(0, 0, 1.0)]
        ex = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0],
                                partition_extractor=lambda r: r[1],
                                value_extractor=lambda r: r[2])
        pre_ex = pdp.PreAggregateExtractors(partition_extractor=lambda r: r[0],
                                            preaggregate_extractor=lambda r: r[1])
        tune_options = parameter_tuning.TuneOptions(
            epsilon=1.0, delta=1e-6, aggregate_params=params,
            function_to_minimize=parameter_tuning.MinimizingFunction.ABSOLUTE_ERROR,
            parameters_to_tune=parameter_tuning.ParametersToTune(max_partitions_contributed=True))
        pre_options = analysis.UtilityAnalysisOptions(epsilon=1.0, delta=1e-6,
                                                      aggregate_params=params,
                                                      pre_aggregated_data=True)
        engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(1.0, 1e-6), backend)
        bounds_params = pdp.CalculatePrivateContributionBoundsParams(
            aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=1.0,
            aggregation_delta=0.0, calculation_eps=1.0, max_partitions_contributed_upper_bound=3)
        calls = {
            "tune": lambda: parameter_tuning.tune(rows, backend, None, tune_options, ex),
            "histograms": lambda: computing_histograms.compute_dataset_histograms(rows, ex,
                                                                                  backend),
            "histograms_pre": lambda: (
                computing_histograms.compute_dataset_histograms_on_preaggregated_data(
                    [(0, (1, 1.0, 1))], pre_ex, backend)),
            "pre_aggregated_data": lambda: analysis.perform_utility_analysis(
                [(0, (1, 1.0, 1))], backend, pre_options, pre_ex),
            "private_bounds": lambda: engine.calculate_private_contribution_bounds(
                rows, bounds_params, ex, [0]),
        }
        got = {}
        for name, call in calls.items():
            try:
                call()
                got[name] = "no error"
            except NotImplementedError as e:
                got[name] = f"NotImplementedError: {e}"
            except Exception as e:  # reported by the test
                got[name] = f"{type(e).__name__}: {e}"
        got["context_created"] = backend._ctx is not None
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, worker):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
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
    return res


@pytest.mark.parametrize("world", [2, 3, 4])
def test_exchange_owner_pairs_gloo(world):
    res = _run(world, _worker)
    everything = np.concatenate([_local(world, r) for r in range(world)])  # rank order
    everything = everything[np.argsort(everything["pk"], kind="stable")]
    assert len(_local(world, world - 1)) == 0 and P % world != 0
    seen = 0
    for rank, pairs, starts, n_local, n, n_bad in res:
        want = everything[everything["pk"] % world == rank].copy()
        want["pk"] //= world
        assert n_local == len(range(rank, P, world))
        assert n_bad == 0 and n == len(want) > 0
        assert pairs[:n].tobytes() == _words(want).tobytes()  # all 24 bytes of every entry
        assert np.array_equal(starts, np.searchsorted(want["pk"], np.arange(n_local + 1)))
        seen += n
    assert seen == N


def test_one_process_calls_raise_on_two_ranks():
    res = _run(2, _guard_worker)
    assert res[0][1] == res[1][1]  # identically on every rank
    got = res[0][1]
    assert got.pop("context_created") is False  # before any device work
    assert set(got) == {"tune", "histograms", "histograms_pre", "pre_aggregated_data",
                        "private_bounds"}
    for name, outcome in got.items():
        assert outcome.startswith("NotImplementedError") and "world_size > 1" in outcome, \
            (name, outcome)
