"""DPEngine.aggregate with VECTOR_SUM on the GPU: the vector columns are the
clipped (and noised) sums of the restated kept set's rows
(tests/percentile_ref.py, tests/vector_ref.py), and the other columns and the
kept partitions are those of the same release without the vector."""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from tests import vector_ref as ref

pytestmark = pytest.mark.gpu

SEED, NONCE = 0x5EED, 31337
P, D = 50, 5
BIG = 1e9  # a norm bound no sum reaches


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(23)
    n = 20_000
    pid = rng.integers(0, 2_000, n).astype(np.int64)
    pk = ((rng.zipf(1.3, n) - 1) % P).astype(np.int64)
    return pid, pk, rng.integers(-3, 14, (n, D)).astype(np.float64)


def _release(built, data, metrics, eps, public=None, noise=False, n_partitions=P,
             norm=pdp.NormKind.Linf, max_norm=BIG, noise_kind=pdp.NoiseKind.LAPLACE, **kw):
    pid, pk, val = data
    vec = pdp.Metrics.VECTOR_SUM in metrics  # opt in only where the vector is asked for
    backend = pdp.MI355XBackend(device=0, seed=SEED, vector_sums=vec)
    acc = pdp.NaiveBudgetAccountant(eps, 1e-5)
    vkw = dict(vector_size=D, vector_max_norm=max_norm, vector_norm_kind=norm) if vec else {}
    params = pdp.AggregateParams(metrics=metrics, max_partitions_contributed=3,
                                 max_contributions_per_partition=2, noise_kind=noise_kind,
                                 **vkw, **kw)
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


def test_public_partitions(built, data):
    """Public partitions, one of them absent from the data; noise off and a
    norm bound out of reach: the columns are the kept rows' sums."""
    pid, pk, val = data
    public = list(range(0, P, 2)) + [P]
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM], 1.0,
                              public, n_partitions=P + 1)
    assert res.plan.fields == ("count", "vector_sum")
    assert ids.tolist() == sorted(public) and vals.shape == (len(public), 1 + D)
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED, public)
    assert np.array_equal(res.last_record_keep.cpu().numpy(), keep)
    want = ref.partition_sums(pk, val, keep, P + 1)
    assert np.array_equal(res.last_vector_sums.cpu().numpy(), want)
    assert np.array_equal(vals[:, 1:], want[ids])
    assert (vals[-1, 1:] == 0.0).all() and np.abs(vals[:-1, 1:]).sum() > 0  # the absent one
    assert np.array_equal(vals[:, 0], np.bincount(pk[keep == 1], minlength=P + 1)[ids])
    # the vector does not disturb the other columns
    _, ids0, vals0 = _release(built, data, [pdp.Metrics.COUNT], 1.0, public, n_partitions=P + 1)
    assert np.array_equal(ids0, ids) and np.array_equal(vals0[:, 0], vals[:, 0])
    # the MetricsTuple of the lazy collection
    key, first = next(iter(res))
    assert first._fields == res.plan.fields
    assert isinstance(first.count, float)
    assert isinstance(first.vector_sum, np.ndarray) and first.vector_sum.dtype == np.float64
    assert first.vector_sum.shape == (D,)
    k0 = res.materialize().partition_ids.cpu().numpy()[0]
    assert key == k0 and np.array_equal(first.vector_sum, want[k0])


def test_l2_clip(built, data):
    pid, pk, val = data
    public = list(range(P))
    res0, ids, raw = _release(built, data, [pdp.Metrics.VECTOR_SUM], 1.0, public)
    norms = np.sqrt((raw * raw).sum(1))
    max_norm = float(np.median(norms))
    assert (norms > max_norm).any() and (norms <= max_norm).any()
    res, ids, vals = _release(built, data, [pdp.Metrics.VECTOR_SUM], 1.0, public,
                              norm=pdp.NormKind.L2, max_norm=max_norm)
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED, public)
    sums = ref.partition_sums(pk, val, keep, P)
    want = np.stack([ref.clip(r, max_norm, ref.NORM_L2) for r in sums])
    assert np.allclose(vals, want[ids], rtol=1e-12, atol=0)


@pytest.mark.parametrize("noise_kind", [pdp.NoiseKind.LAPLACE, pdp.NoiseKind.GAUSSIAN],
                         ids=["laplace", "gaussian"])
def test_private_selection_and_keyed_noise(built, data, noise_kind):
    """Private selection with noise on.  Three equal budget requests of a
    total epsilon of 3 (count, vector, selection) against two of a total of 2
    (count, selection): the same selection and count budgets, so with the
    same nonce the kept partitions and the noised count agree exactly
    (Laplace).  The vector columns are the oracle's sampler on the clipped
    sums, for both noise kinds."""
    from oracle import oracle
    pid, pk, val = data
    max_norm = 2000.0  # the l1 norms of the kept sums run from about 900 to 37000
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM], 3.0,
                              noise=True, norm=pdp.NormKind.L1, max_norm=max_norm,
                              noise_kind=noise_kind)
    assert 0 < len(ids) <= P
    if noise_kind == pdp.NoiseKind.LAPLACE:
        # (Gaussian mechanisms share delta as well: a third request changes the others')
        _, ids0, vals0 = _release(built, data, [pdp.Metrics.COUNT], 2.0, noise=True,
                                  noise_kind=noise_kind)
        assert np.array_equal(ids0, ids) and np.array_equal(vals0[:, 0], vals[:, 0])
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED)
    sums = ref.partition_sums(pk, val, keep, P)
    assert np.array_equal(res.last_vector_sums.cpu().numpy(), sums)
    l1 = np.abs(sums).sum(1)
    assert (l1[ids] > max_norm).any() and (l1[ids] <= max_norm).any()
    f = res.plan.vector_fields(True)
    ss = oracle.stream_seed(SEED, NONCE)
    for k, row in zip(ids.tolist(), vals[:, 1:]):
        clipped = ref.clip(sums[k], max_norm, ref.NORM_L1)
        noised = ref.oracle_noise(f["noise_kind"], f["scale"], ss, k)
        want = np.array([noised(d, clipped[d]) for d in range(D)])
        assert np.allclose(row, want, rtol=1e-12, atol=1e-6), (k, row, want)
    assert (np.abs(vals[:, 1:] - np.stack([ref.clip(sums[k], max_norm, ref.NORM_L1)
                                           for k in ids])) > 1e-3).mean() > 0.5


def test_vector_sum_alone(built, data):
    pid, pk, val = data
    res, ids, vals = _release(built, data, [pdp.Metrics.VECTOR_SUM], 1.0, list(range(P)))
    assert res.plan.fields == ("vector_sum",) and res.plan.mask == 0 and vals.shape == (P, D)
    keep = ref.kept_records(pid, pk, res.last_bound_fields, SEED, range(P))
    assert np.array_equal(vals, ref.partition_sums(pk, val, keep, P))


def test_contribution_bounds_already_enforced(built, data):
    """Every row is its own privacy unit: every record is kept."""
    pid, pk, val = data
    res, ids, vals = _release(built, data, [pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM], 1.0,
                              list(range(P)), contribution_bounds_already_enforced=True)
    assert res.last_record_keep.all()
    assert np.array_equal(vals[:, 0], np.bincount(pk, minlength=P))
    assert np.array_equal(vals[:, 1:], ref.partition_sums(pk, val, np.ones(len(pk)), P))


def _small(built, col, ex):
    backend = pdp.MI355XBackend(device=0, seed=SEED, vector_sums=True)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-5)
    params = pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM],
                                 max_partitions_contributed=3, max_contributions_per_partition=2,
                                 vector_size=D, vector_max_norm=BIG,
                                 vector_norm_kind=pdp.NormKind.Linf)
    res = pdp.DPEngine(acc, backend).aggregate(col, params, ex, public_partitions=list(range(P)))
    acc.compute_budgets()
    res.noise_enabled = False
    res.nonce = NONCE
    return res


def test_row_input_equals_columnar(built, data):
    """200 rows as tuples whose value is a sequence of D numbers."""
    pid, pk, val = (x[:200] for x in data)
    rows = [(int(a), int(b), tuple(v.tolist())) for a, b, v in zip(pid, pk, val)]
    r = _small(built, rows, pdp.DataExtractors(lambda r: r[0], lambda r: r[1], lambda r: r[2]))
    got = {k: t for k, t in r}
    col = pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                           value=torch.as_tensor(val))
    c = _small(built, col, pdp.DataExtractors("pid", "pk", "value"))
    want = {k: t for k, t in c}
    assert sorted(got) == sorted(want) == list(range(P))
    assert any(t.count > 0 for t in want.values())
    for k in want:
        assert got[k].count == want[k].count
        assert np.array_equal(got[k].vector_sum, want[k].vector_sum)


def test_shape_mismatch_raises(built, data):
    pid, pk, val = (x[:200] for x in data)
    wide = np.concatenate([val, val[:, :1]], axis=1)  # (n, D + 1)
    col = pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                           value=torch.as_tensor(wide))
    with pytest.raises(TypeError, match="Shape mismatch"):
        _small(built, col, pdp.DataExtractors("pid", "pk", "value")).materialize()
    col = pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                           value=torch.as_tensor(val[:, 0].copy()))  # scalars
    with pytest.raises(TypeError, match="Shape mismatch"):
        _small(built, col, pdp.DataExtractors("pid", "pk", "value")).materialize()
