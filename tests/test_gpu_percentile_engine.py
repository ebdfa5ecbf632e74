"""DPEngine.aggregate with PERCENTILE metrics on the GPU: the percentile
columns equal the restated walk over the restated kept set
(tests/percentile_ref.py), and the other columns and the kept partitions are
those of the same release without percentiles."""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from tests import percentile_ref as ref

pytestmark = pytest.mark.gpu

SEED, NONCE = 0x5EED, 31337
P, LO, HI = 50, 0.0, 64.0
TOL = 1e-12 * (HI - LO)
PCT = [pdp.Metrics.PERCENTILE(50), pdp.Metrics.PERCENTILE(90)]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(23)
    n = 20_000
    pid = rng.integers(0, 2_000, n).astype(np.int64)
    pk = ((rng.zipf(1.3, n) - 1) % P).astype(np.int64)
    return pid, pk, rng.uniform(LO - 4.0, HI + 4.0, n)


def _release(built, data, metrics, eps, public=None, noise=False, n_partitions=P, **kw):
    pid, pk, val = data
    pct = any(m.is_percentile for m in metrics)  # opt in only where percentiles are asked for
    backend = pdp.MI355XBackend(device=0, seed=SEED, percentiles=pct)
    acc = pdp.NaiveBudgetAccountant(eps, 1e-5)
    params = pdp.AggregateParams(metrics=metrics, max_partitions_contributed=3,
                                 max_contributions_per_partition=2, min_value=LO, max_value=HI,
                                 **kw)
    if kw.get("contribution_bounds_already_enforced"):
        col = pdp.ColumnarData(pk=torch.as_tensor(pk), value=torch.as_tensor(val),
                               n_partitions=n_partitions)
        ex = pdp.DataExtractors(partition_extractor="pk", value_extractor="value")
    else:
        col = pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                               value=torch.as_tensor(val), n_partitions=n_partitions)
        ex = pdp.DataExtractors("pid", "pk", "value")
    res = pdp.DPEngine(acc, backend).aggregate(col, params, ex, public_partitions=public)
    acc.compute_budgets()
    res.noise_enabled = noise
    res.nonce = NONCE
    out = res.materialize()
    ids = out.partition_ids.cpu().numpy()
    o = np.argsort(ids)
    return res, ids[o], out.values.cpu().numpy()[o]


def _check_percentiles(data, keep, ids, cols, qs):
    pid, pk, val = data
    for k, row in zip(ids.tolist(), cols):
        want, margin = ref.quantiles(val[(pk == k) & (keep == 1)], qs, LO, HI)
        assert margin >= 1e-9
        assert np.abs(row - want).max() <= TOL, (k, row, want)


def test_public_partitions(built, data):
    """Public partitions, one of them absent from the data; noise off."""
    pid, pk, val = data
    public = list(range(0, P, 2)) + [P]
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT] + PCT, 1.0, public,
                              n_partitions=P + 1)
    assert res.plan.fields == ("count", "percentile_50", "percentile_90")
    assert res.plan.MetricsTuple._fields == res.plan.fields
    assert ids.tolist() == sorted(public) and vals.shape == (len(public), 3)
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED, public)
    assert np.array_equal(res.last_record_keep.cpu().numpy(), keep)
    assert np.array_equal(vals[:, 0], np.bincount(pk[keep == 1], minlength=P + 1)[ids])
    _check_percentiles(data, keep, ids, vals[:, 1:], [0.5, 0.9])
    # the absent partition: an empty tree
    assert np.abs(vals[-1, 1:] - (LO + np.array([0.5, 0.9]) * (HI - LO))).max() <= TOL
    # the percentiles do not disturb the other columns
    _, ids0, vals0 = _release(built, data, [pdp.Metrics.COUNT], 1.0, public, n_partitions=P + 1)
    assert np.array_equal(ids0, ids) and np.array_equal(vals0[:, 0], vals[:, 0])
    # the MetricsTuple of the lazy collection
    first = next(iter(res))[1]
    assert first._fields == res.plan.fields


def test_private_selection_keeps_partitions_and_count(built, data):
    """Private selection with noise on.  Three equal budget requests of a
    total epsilon of 3 (count, percentiles, selection) against two of a total
    of 2 (count, selection): the same selection and count budgets, so with
    the same nonce the kept partitions and the noised count agree exactly."""
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT] + PCT, 3.0, noise=True)
    _, ids0, vals0 = _release(built, data, [pdp.Metrics.COUNT], 2.0, noise=True)
    assert 0 < len(ids) <= P
    assert np.array_equal(ids0, ids) and np.array_equal(vals0[:, 0], vals[:, 0])
    assert ((vals[:, 1:] >= LO) & (vals[:, 1:] <= HI)).all()
    assert (vals[:, 1] <= vals[:, 2]).mean() > 0.9  # noisy, but the median sits below p90
    # noise off: the restated walk over the restated kept set
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT] + PCT, 3.0)
    pid, pk, val = data
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED)
    _check_percentiles(data, keep, ids, vals[:, 1:], [0.5, 0.9])


def test_percentiles_alone(built, data):
    pid, pk, val = data
    res, ids, vals = _release(built, data, [pdp.Metrics.PERCENTILE(12.5)], 1.0, list(range(P)))
    assert res.plan.fields == ("percentile_12_5",) and vals.shape == (P, 1)
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED, range(P))
    _check_percentiles(data, keep, ids, vals, [0.125])


def test_contribution_bounds_already_enforced(built, data):
    """Every row is its own privacy unit: every record is kept."""
    pid, pk, val = data
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT] + PCT, 1.0, list(range(P)),
                              contribution_bounds_already_enforced=True)
    assert res.last_record_keep.all()
    assert np.array_equal(vals[:, 0], np.bincount(pk, minlength=P))
    _check_percentiles(data, np.ones(len(pk), np.uint8), ids, vals[:, 1:], [0.5, 0.9])
