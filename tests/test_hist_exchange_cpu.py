"""The collectives of the multi-rank dataset histograms on host tensors over
gloo (no GPU): distributed.hist_header and distributed.merge_histograms with
three ranks, one of them holding nothing, against numpy; an error flag on one
rank raises on every rank; a dataset without pairs keeps its empty range; and
the three public calls accept ColumnarData(n_partitions=P) on two ranks --
lazily, before any device work."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

T, NB, NS = 5, 40, 30
WORLD = 3


def _bins(rank):
    """Synthetic bins of one rank (rank 2: all zero): (int_bins, sum_count,
    sum_sum, sum_max, range)."""
    ib = np.zeros((T, NB, 3), np.int64)
    sc, ss, sm = np.zeros(NS, np.int64), np.zeros(NS), np.zeros(NS)
    rng = np.array([np.inf, -np.inf])
    if rank < 2:
        g = np.random.default_rng(100 + rank)
        on = g.integers(0, 2, (T, NB)).astype(bool)
        ib[..., 0] = g.integers(1, 50, (T, NB)) * on
        ib[..., 1] = ib[..., 0] * g.integers(1, 1 << 40, (T, NB))
        ib[..., 2] = g.integers(1, 1 << 62, (T, NB)) * on
        sc[:] = g.integers(0, 3, NS)
        # negative sums: a maximum of 0.0 from a rank's empty bin must not win
        sm[:] = np.where(sc > 0, -g.uniform(0.5, 9.0, NS) * (1 + np.arange(NS) % 2 * -2), 0.0)
        ss[:] = np.where(sc > 0, sm * sc, 0.0)
        rng = np.array([-3.5 - rank, 2.25 + 4 * rank])
    return ib, sc, ss, sm, rng


def _merge_worker(rank, world, port, q):
    import torch.distributed as dist
    from pipelinedp_amd import distributed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.group.WORLD
        ib, sc, ss, sm, rng = (torch.from_numpy(a) for a in _bins(rank))
        got = {}
        r, bound = distributed.hist_header(rng, 10 * (rank + 1), group)
        got["header"] = (r.tolist(), bound)
        r, bound = distributed.hist_header(torch.tensor([np.inf, -np.inf], dtype=torch.float64),
                                           0, group)
        got["empty_header"] = (r.tolist(), bound)
        out = distributed.merge_histograms(ib, sc, ss, sm, torch.zeros(1, dtype=torch.float64),
                                           group)
        got["merged"] = [t.numpy() for t in out]
        zero = distributed.merge_histograms(torch.zeros_like(ib), torch.zeros_like(sc),
                                            torch.zeros_like(ss), torch.zeros_like(sm), None,
                                            group)
        got["nothing"] = all(not t.any() for t in zero)
        try:  # rank 1 alone reports an error
            distributed.merge_histograms(ib, sc, ss, sm,
                                         torch.tensor([2.0 if rank == 1 else 0.0]), group)
            got["flag"] = "no error"
        except RuntimeError as e:
            got["flag"] = f"RuntimeError: {e}"
        # the ranks went on together after the error
        got["after"] = distributed.hist_header(rng, 1, group)[1]
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def _entry_worker(rank, world, port, q):
    import torch.distributed as dist
    import pipelinedp_amd as pdp
    from pipelinedp_amd.analysis import parameter_tuning
    from pipelinedp_amd.dataset_histograms import computing_histograms
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        backend = pdp.MI355XBackend(device=0, seed=1, process_group=dist.group.WORLD)
        params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                     max_partitions_contributed=1,
                                     max_contributions_per_partition=1)
        col = pdp.ColumnarData(pid=torch.tensor([0, 1]), pk=torch.tensor([0, 2]),
                               value=torch.tensor([1.0, 2.0]), n_partitions=4)
        undeclared = pdp.ColumnarData(pid=torch.tensor([0, 1]), pk=torch.tensor([0, 2]),
                                      value=torch.tensor([1.0, 2.0]))
        ex = pdp.DataExtractors("pid", "pk", "value")
        engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(1.0, 1e-6), backend)
        bounds_params = pdp.CalculatePrivateContributionBoundsParams(
            aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=1.0,
            aggregation_delta=0.0, calculation_eps=1.0, max_partitions_contributed_upper_bound=3)
        calls = {
            "histograms": lambda c: computing_histograms.compute_dataset_histograms(c, ex, backend),
            "private_bounds": lambda c: engine.calculate_private_contribution_bounds(
                c, bounds_params, ex, [0, 2]),
        }
        got = {}
        for name, call in calls.items():
            for tag, c in (("declared", col), ("undeclared", undeclared)):
                try:
                    got[f"{name}/{tag}"] = type(call(c)).__name__
                except NotImplementedError as e:
                    got[f"{name}/{tag}"] = f"NotImplementedError: {e}"
        tune_options = parameter_tuning.TuneOptions(
            epsilon=1.0, delta=1e-6, aggregate_params=params,
            function_to_minimize=parameter_tuning.MinimizingFunction.ABSOLUTE_ERROR,
            parameters_to_tune=parameter_tuning.ParametersToTune(max_partitions_contributed=True))
        try:
            parameter_tuning.tune(undeclared, backend, None, tune_options, ex)
            got["tune/undeclared"] = "no error"
        except NotImplementedError as e:
            got["tune/undeclared"] = f"NotImplementedError: {e}"
        got["context_created"] = backend._ctx is not None
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def _tune_worker(rank, world, port, q):
    """tune with a declared input: rank 0's candidates reach every rank (the
    ranks are handed different histograms); the lazy results are not run."""
    import torch.distributed as dist
    import pipelinedp_amd as pdp
    from pipelinedp_amd.analysis import parameter_tuning
    from pipelinedp_amd.dataset_histograms import histograms as hist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        backend = pdp.MI355XBackend(device=0, seed=1, process_group=dist.group.WORLD)
        params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                     max_partitions_contributed=1,
                                     max_contributions_per_partition=1)
        col = pdp.ColumnarData(pid=torch.tensor([0, 1]), pk=torch.tensor([0, 2]),
                               value=torch.tensor([1.0, 2.0]), n_partitions=4)
        top = 5 + 4 * rank  # L0 up to 5 on rank 0, 9 on rank 1
        l0 = hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS,
                            [hist.FrequencyBin(lower=v, upper=v + 1, count=1, sum=v, max=v)
                             for v in range(1, top + 1)])
        hs = hist.DatasetHistograms(l0, None, None, None, None, None)
        options = parameter_tuning.TuneOptions(
            epsilon=1.0, delta=1e-6, aggregate_params=params,
            function_to_minimize=parameter_tuning.MinimizingFunction.ABSOLUTE_ERROR,
            parameters_to_tune=parameter_tuning.ParametersToTune(max_partitions_contributed=True))
        seen = {}
        real = parameter_tuning.utility_analysis.perform_utility_analysis

        def spy(col_, backend_, ua_options, *a, **k):
            seen["l0"] = list(ua_options.multi_param_configuration.max_partitions_contributed)
            return iter(()), iter(())

        parameter_tuning.utility_analysis.perform_utility_analysis = spy
        try:
            parameter_tuning.tune(col, backend, hs, options, pdp.DataExtractors("pid", "pk", "value"))
        finally:
            parameter_tuning.utility_analysis.perform_utility_analysis = real
        q.put((rank, dict(l0=seen["l0"], context_created=backend._ctx is not None)))
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
    return [r[1] for r in res]


@pytest.fixture(scope="module")
def merged():
    return _run(WORLD, _merge_worker)


def test_header_is_the_range_and_the_largest_bound(merged):
    for got in merged:
        assert got["header"] == ([-4.5, 6.25], 30)
        assert got["empty_header"] == ([np.inf, -np.inf], 0)


def test_merge_sums_and_maxima(merged):
    parts = [_bins(r) for r in range(WORLD)]
    ib = np.stack([p[0] for p in parts])
    want_ib = np.concatenate([ib[..., 0:2].sum(0), ib[..., 2:3].max(0)], -1)
    want_sc = sum(p[1] for p in parts)
    want_ss = sum(p[2] for p in parts)
    masked = np.stack([np.where(p[1] > 0, p[3], -np.inf) for p in parts]).max(0)
    want_sm = np.where(want_sc > 0, masked, 0.0)
    assert (want_sm < 0).any() and (want_sm > 0).any() and (want_sc == 0).any()
    for got in merged:
        g_ib, g_sc, g_ss, g_sm = got["merged"]
        assert np.array_equal(g_ib, want_ib) and np.array_equal(g_sc, want_sc)
        assert g_sm.tobytes() == want_sm.tobytes()  # the maxima's bits
        assert np.allclose(g_ss, want_ss, rtol=1e-15, atol=0)
        assert np.array_equal(g_ss, merged[0]["merged"][2])  # the same on every rank
        assert got["nothing"] is True


def test_a_flag_on_one_rank_raises_on_every_rank(merged):
    for got in merged:
        assert got["flag"].startswith("RuntimeError") and "1 ranks" in got["flag"], got["flag"]
        assert got["after"] == 1


def test_declared_partitions_are_accepted_lazily():
    res = _run(2, _entry_worker)
    assert res[0] == res[1]
    got = res[0]
    assert got.pop("context_created") is False  # host state only
    for name in ("histograms", "private_bounds"):
        assert got[f"{name}/declared"] == "_OneElement"
    for name in ("histograms", "private_bounds", "tune"):
        out = got[f"{name}/undeclared"]
        assert out.startswith("NotImplementedError") and "world_size > 1" in out, out
        assert "n_partitions" in out


def test_tune_broadcasts_rank_zeros_candidates():
    res = _run(2, _tune_worker)
    assert res[0]["l0"] == res[1]["l0"] == [1, 2, 3, 4, 5]
    assert not res[0]["context_created"] and not res[1]["context_created"]
