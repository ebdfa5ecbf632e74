"""CompoundPlan with PERCENTILE metrics (host only): fields, budget requests
and the tree's noise scale; what stays unsupported still raises."""
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import combiners
from pipelinedp_amd import dp_computations as dpc


def _plan(noise_kind, weight=2.0, metrics=None):
    acc = pdp.NaiveBudgetAccountant(1.5, 1e-6)
    specs = []
    orig = acc.request_budget

    def rec(*a, **k):
        s = orig(*a, **k)
        specs.append((s, k.get("weight")))
        return s
    acc.request_budget = rec
    params = pdp.AggregateParams(
        metrics=metrics or [pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50),
                            pdp.Metrics.PERCENTILE(90.5)],
        noise_kind=noise_kind, max_partitions_contributed=3,
        max_contributions_per_partition=2, min_value=0.0, max_value=10.0,
        budget_weight=weight)
    return acc, combiners.CompoundPlan(params, acc), specs


def test_fields_requests_and_laplace_scale():
    acc, plan, specs = _plan(pdp.NoiseKind.LAPLACE)
    assert plan.fields == ("count", "percentile_50", "percentile_90_5")
    assert plan.MetricsTuple._fields == plan.fields
    assert [w for _, w in specs] == [2.0, 2.0]
    assert all(s.mechanism_type == pdp.MechanismType.LAPLACE for s, _ in specs)
    assert plan.expects_per_partition_sampling() and plan.needs_values()
    assert plan.bounding_mode() == combiners.MODE_CROSS_AND_PER
    acc.compute_budgets()
    eps = specs[1][0].eps
    assert eps == pytest.approx(0.75, rel=1e-12)  # two equal weights
    q = plan.quantile_fields(True)
    assert q["scale"] == pytest.approx(3 * 4 * 2 / eps, rel=1e-12)  # mpc * H * mcpp / eps
    assert q["quantiles"] == [0.5, 0.905] and q["n_quantiles"] == 2
    assert (q["lo"], q["hi"]) == (0.0, 10.0)
    assert q["noise_kind"] == combiners.NOISE_LAPLACE
    assert plan.quantile_fields(False)["noise_kind"] == combiners.NOISE_NONE
    # the noise kernel keeps its own columns only
    assert plan.noise_fields()["n_outputs"] == 1
    report = [s() for s in plan.explain_computation()]
    assert report[-1] == f"Computed percentiles [50, 90.5] with (eps={eps} delta={specs[1][0].delta})"


def test_gaussian_sigma_is_the_additive_mechanisms():
    acc, plan, specs = _plan(pdp.NoiseKind.GAUSSIAN)
    acc.compute_budgets()
    spec = specs[1][0]
    want = dpc.AdditiveMechanism(pdp.NoiseKind.GAUSSIAN, spec.eps, spec.delta,
                                 dpc.Sensitivities(l0=4 * 3, linf=2))
    assert plan.quantile_fields()["scale"] == want.scale
    assert plan.quantile_fields()["noise_kind"] == combiners.NOISE_GAUSSIAN


def test_percentiles_alone_and_field_order():
    _, plan, specs = _plan(pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.PERCENTILE(10)])
    assert plan.fields == ("percentile_10",) and plan.mask == 0 and len(specs) == 1
    # after every other field, in the order of params.metrics; the budget
    # request comes after the privacy_id_count one
    _, plan, specs = _plan(pdp.NoiseKind.LAPLACE,
                           metrics=[pdp.Metrics.PERCENTILE(99), pdp.Metrics.PRIVACY_ID_COUNT,
                                    pdp.Metrics.PERCENTILE(1), pdp.Metrics.SUM])
    assert plan.fields == ("sum", "privacy_id_count", "percentile_99", "percentile_1")
    assert list(plan.specs) == ["sum", "privacy_id_count", "percentile"]


EX = pdp.DataExtractors(lambda r: r[0], lambda r: r[1], lambda r: r[2])


def test_engine_needs_the_backend_opt_in():
    """Without MI355XBackend(percentiles=True) the engine raises as before and
    requests no budget; with it, it returns the lazy device plan."""
    params = pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50)],
                                 max_partitions_contributed=1, max_contributions_per_partition=1,
                                 min_value=0.0, max_value=1.0)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    with pytest.raises(NotImplementedError, match="percentiles=True"):
        pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=1)).aggregate(
            [(1, 1, 0.5)], params, EX)
    assert not acc._mechanisms
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    eng = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=1, percentiles=True))
    res = eng.aggregate([(1, 1, 0.5)], params, EX)
    assert res.plan.fields == ("count", "percentile_50")
    acc.compute_budgets()
    assert "Computed percentiles [50]" in eng.explain_computations_report()[0]


def test_max_contributions_with_percentile_still_raises():
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    eng = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=1, percentiles=True))
    params = pdp.AggregateParams(metrics=[pdp.Metrics.PERCENTILE(50)], max_contributions=3,
                                 min_value=0.0, max_value=1.0)
    with pytest.raises(NotImplementedError, match="max_contributions"):
        eng.aggregate([(1, 1, 0.5)], params,
                      pdp.DataExtractors(lambda r: r[0], lambda r: r[1], lambda r: r[2]))


def test_vector_sum_still_raises():
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    params = pdp.AggregateParams(metrics=[pdp.Metrics.VECTOR_SUM], max_partitions_contributed=1,
                                 max_contributions_per_partition=1, vector_size=2,
                                 vector_max_norm=1.0)
    with pytest.raises(NotImplementedError):
        combiners.CompoundPlan(params, acc)
