"""CompoundPlan with VECTOR_SUM (host only): the opt-in, fields, budget
requests, the reference's per-coordinate noise scale, what still raises, and
the numpy clip the GPU tests compare against."""
import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import combiners
from pipelinedp_amd import dp_computations as dpc
from tests import vector_ref as ref

D, MPC, MCPP = 5, 3, 2


def _plan(noise_kind, metrics=None, weight=2.0, **kw):
    acc = pdp.NaiveBudgetAccountant(1.5, 1e-6)
    specs = []
    orig = acc.request_budget

    def rec(*a, **k):
        s = orig(*a, **k)
        specs.append((s, k.get("weight")))
        return s
    acc.request_budget = rec
    vec = dict(vector_size=D, vector_max_norm=4.0, vector_norm_kind=pdp.NormKind.L2)
    vec.update(kw)
    params = pdp.AggregateParams(
        metrics=metrics or [pdp.Metrics.COUNT, pdp.Metrics.PRIVACY_ID_COUNT,
                            pdp.Metrics.VECTOR_SUM],
        noise_kind=noise_kind, max_partitions_contributed=MPC,
        max_contributions_per_partition=MCPP, budget_weight=weight, **vec)
    return acc, combiners.CompoundPlan(params, acc, vector_sums=True), specs


@pytest.mark.parametrize("kind", [pdp.NoiseKind.LAPLACE, pdp.NoiseKind.GAUSSIAN],
                         ids=["laplace", "gaussian"])
def test_fields_requests_and_scale(kind):
    acc, plan, specs = _plan(kind)
    assert plan.fields == ("count", "privacy_id_count", "vector_sum")
    assert plan.MetricsTuple._fields == plan.fields
    assert list(plan.specs) == ["count", "privacy_id_count", "vector_sum"]
    assert [w for _, w in specs] == [2.0, 2.0, 2.0]
    assert all(s.mechanism_type == kind.convert_to_mechanism_type() for s, _ in specs)
    assert plan.vector_size == D
    assert plan.needs_values() and plan.expects_per_partition_sampling()
    assert plan.bounding_mode() == combiners.MODE_CROSS_AND_PER
    acc.compute_budgets()
    eps = [s.eps for s, _ in specs]
    assert eps[0] == pytest.approx(0.5, rel=1e-12) and eps[0] == eps[1] == eps[2]
    spec = specs[2][0]
    v = plan.vector_fields(True)
    assert v["scale"] == dpc.noise_scale(kind, spec.eps / D, spec.delta / D, MPC, MCPP)
    if kind == pdp.NoiseKind.LAPLACE:
        assert v["scale"] == pytest.approx(MPC * MCPP * D / spec.eps, rel=1e-12)
    assert v["size"] == D and v["max_norm"] == 4.0 and v["norm_kind"] == combiners.NORM_L2
    assert v["noise_kind"] == (combiners.NOISE_LAPLACE if kind == pdp.NoiseKind.LAPLACE
                               else combiners.NOISE_GAUSSIAN)
    assert plan.vector_fields(False)["noise_kind"] == combiners.NOISE_NONE
    assert set(v) == {"size", "norm_kind", "max_norm", "noise_kind", "scale"}
    # the noise kernel keeps its own columns only
    nf = plan.noise_fields()
    assert nf["n_outputs"] == 2 and nf["out_src"][:2] == [combiners.V_COUNT, combiners.V_PID]
    # the reference's combiner explains nothing
    assert len(plan.explain_computation()) == 2


def test_vector_sum_alone_and_norm_kinds():
    for nk, want in ((pdp.NormKind.Linf, combiners.NORM_LINF), (pdp.NormKind.L1, combiners.NORM_L1),
                     (pdp.NormKind.L2, combiners.NORM_L2)):
        acc, plan, specs = _plan(pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.VECTOR_SUM],
                                 vector_norm_kind=nk)
        assert plan.fields == ("vector_sum",) and plan.mask == 0 and len(specs) == 1
        assert plan.n_noise_outputs == 0
        acc.compute_budgets()
        assert plan.vector_fields()["norm_kind"] == want


def test_vector_sum_with_percentile_raises():
    with pytest.raises(NotImplementedError, match="PERCENTILE"):
        _plan(pdp.NoiseKind.LAPLACE,
              metrics=[pdp.Metrics.VECTOR_SUM, pdp.Metrics.PERCENTILE(50)])


@pytest.mark.parametrize("missing", ["vector_size", "vector_max_norm", "vector_norm_kind"])
def test_missing_vector_parameter_raises(missing):
    with pytest.raises(ValueError, match=missing):
        _plan(pdp.NoiseKind.LAPLACE, **{missing: None})


EX = pdp.DataExtractors(lambda r: r[0], lambda r: r[1], lambda r: r[2])


def test_engine_needs_the_backend_opt_in():
    """Without MI355XBackend(vector_sums=True) the engine raises and requests
    no budget; with it, it returns the lazy device plan."""
    params = pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM],
                                 max_partitions_contributed=1, max_contributions_per_partition=1,
                                 vector_size=2, vector_max_norm=1.0,
                                 vector_norm_kind=pdp.NormKind.Linf)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    backend = pdp.MI355XBackend(device=0, seed=1)
    assert backend.vector_sums is False
    with pytest.raises(NotImplementedError, match="vector_sums=True"):
        pdp.DPEngine(acc, backend).aggregate([(1, 1, (0.5, 1.0))], params, EX)
    assert not acc._mechanisms
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    eng = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=1, vector_sums=True))
    res = eng.aggregate([(1, 1, (0.5, 1.0))], params, EX)
    assert res.plan.fields == ("count", "vector_sum") and res.plan.vector_size == 2
    acc.compute_budgets()
    assert "Computed DP count" in eng.explain_computations_report()[0]


def test_max_contributions_with_vector_sum_still_raises():
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    eng = pdp.DPEngine(acc, pdp.MI355XBackend(device=0, seed=1, vector_sums=True))
    params = pdp.AggregateParams(metrics=[pdp.Metrics.VECTOR_SUM], max_contributions=3,
                                 vector_size=2, vector_max_norm=1.0,
                                 vector_norm_kind=pdp.NormKind.Linf)
    with pytest.raises(NotImplementedError, match="max_contributions"):
        eng.aggregate([(1, 1, (0.5, 1.0))], params, EX)


def test_reference_clip_by_hand():
    s = np.array([3.0, -4.0, 12.0])  # l1 19, l2 13, linf 12
    assert np.array_equal(ref.clip(s, 5.0, ref.NORM_LINF), [3.0, -4.0, 5.0])
    assert np.array_equal(ref.clip(s, 12.0, ref.NORM_LINF), s)
    assert np.allclose(ref.clip(s, 9.5, ref.NORM_L1), s * 0.5, rtol=1e-15, atol=0)
    assert np.allclose(ref.clip(s, 6.5, ref.NORM_L2), [1.5, -2.0, 6.0], rtol=1e-15, atol=0)
    assert np.array_equal(ref.clip(s, 19.0, ref.NORM_L1), s)  # at the norm: untouched
    assert np.array_equal(ref.clip(s, 13.0, ref.NORM_L2), s)
    assert (ref.norm(s, ref.NORM_L1), ref.norm(s, ref.NORM_L2), ref.norm(s, ref.NORM_LINF)) == \
        (19.0, 13.0, 12.0)
    z = np.zeros(3)
    for kind in (ref.NORM_LINF, ref.NORM_L1, ref.NORM_L2):
        c = ref.clip(z, 2.0, kind)
        assert np.isfinite(c).all() and (c == 0.0).all()
