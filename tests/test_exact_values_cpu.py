"""The exact-value convention of tests/exact_values.py, checked on the CPU:
the generator, the oracle's arithmetic against int64 group-bys, its
independence of the record order, and -- for every (mode, input) pair of
tests/test_gpu_mode_matrix.py -- that the contribution and clipping bounds
bind, so that no GPU case compares a path on which nothing happens."""
import numpy as np
import pytest

import pipelinedp_amd as pdp
from oracle import oracle
from pipelinedp_amd import combiners
from tests import exact_values as ev


def _oracle(gen, fields, order=None):
    pid, pk, val, P = ev.dataset(gen)
    rec_ids = None
    if order is not None:
        pid, pk, val, rec_ids = pid[order], pk[order], val[order], order
    return oracle.bound_aggregate(pid, pk, val, fields, ev.SEED,
                                  public_mask=oracle.bitmap(range(P), P) if P <= 20_000 else None,
                                  rec_ids=rec_ids)


def test_generator_range_and_fraction():
    v = ev.exact_values(np.random.default_rng(1), 200_000)
    assert v.dtype == np.float64
    assert v.min() >= ev.V_LO and v.max() < ev.V_HI
    k = v * ev.SCALE
    assert np.array_equal(k, np.rint(k))                      # 12 fraction bits, no more
    assert np.array_equal(ev.to_fixed(v).astype(np.float64) / ev.SCALE, v)
    # the whole range is used, both ends and odd numerators included
    assert v.min() < ev.V_LO + 0.01 and v.max() > ev.V_HI - 0.01
    assert (ev.to_fixed(v) & 1).mean() > 0.4
    with pytest.raises(ValueError):
        ev.to_fixed(np.array([1.0 / 8192]))


def test_bounds_and_midpoints_are_exact():
    """Every clipping bound of the matrix and every value range's midpoint is
    a multiple of 1/4096."""
    for mode, gen in ev.PAIRS:
        kw = ev.params_kwargs(mode, gen)
        for k in ("min_value", "max_value", "min_sum_per_partition", "max_sum_per_partition"):
            if k in kw:
                ev.to_fixed(kw[k])
        if "min_value" in kw:
            ev.to_fixed(kw["min_value"] + (kw["max_value"] - kw["min_value"]) / 2)


def test_inputs_stay_within_the_exact_range():
    for gen in sorted({g for _, g in ev.PAIRS}):
        pid, pk, val, P = ev.dataset(gen)
        assert pid.size == pk.size == val.size <= ev.MAX_RECORDS
        ev.to_fixed(val)
        assert 0 <= pk.min() and pk.max() < P


# ------------------------------------------------------ oracle arithmetic
def _group_sum(keys, weights, P):
    out = np.zeros(P, np.int64)
    np.add.at(out, keys, weights)
    return out


@pytest.mark.parametrize("mode", ["item32", "mean_var", "perpid_var", "cap_sum_pp",
                                  "cross_sum_pp", "perpid_sum_pp"])
def test_oracle_sums_equal_int64_group_by(mode):
    """Non-binding contribution bounds: every record is kept, so the oracle's
    float sums are the exact rationals of an int64 group-by (values x 4096):
    clamp each record then sum per partition (CLIP_VALUE), or sum per pair,
    clamp, then sum per partition (CLIP_PARTITION)."""
    pid, pk, val, P = ev.dataset("small")
    fields = ev.bound_fields(mode, "small")
    big = 1 << 30
    if ev.is_per_pid(mode):
        fields["max_contributions"] = big
    else:
        fields["max_partitions_contributed"] = fields["max_contributions_per_partition"] = big
    ref = _oracle("small", fields)
    k = ev.to_fixed(val)
    assert np.array_equal(ref["count"], np.bincount(pk, minlength=P))
    pair = pid * P + pk
    upair, inv = np.unique(pair, return_inverse=True)
    assert np.array_equal(ref["rows"], np.bincount(upair % P, minlength=P))
    if fields["sum_mode"] == ev.CLIP_PARTITION:
        lo = int(ev.to_fixed(fields["min_sum_per_partition"]))
        hi = int(ev.to_fixed(fields["max_sum_per_partition"]))
        pair_sum = _group_sum(inv, k, upair.size)
        assert (pair_sum < lo).any() and (pair_sum > hi).any()
        want = _group_sum(upair % P, np.clip(pair_sum, lo, hi), P)
        assert np.array_equal(ref["sum"], want.astype(np.float64) / ev.SCALE)
    else:
        lo, hi = int(ev.to_fixed(fields["min_value"])), int(ev.to_fixed(fields["max_value"]))
        mid = int(ev.to_fixed(fields["min_value"]
                              + (fields["max_value"] - fields["min_value"]) / 2))
        x = np.clip(k, lo, hi)
        assert np.array_equal(ref["sum"], _group_sum(pk, x, P).astype(np.float64) / ev.SCALE)
        assert np.array_equal(ref["nsum"],
                              _group_sum(pk, x - mid, P).astype(np.float64) / ev.SCALE)
        nsq = _group_sum(pk, (x - mid) ** 2, P)
        assert nsq.max() < 1 << 53
        assert np.array_equal(ref["nsq"], nsq.astype(np.float64) / ev.SCALE ** 2)


@pytest.mark.parametrize("mode", sorted(ev.MODES))
def test_oracle_is_independent_of_the_record_order(mode):
    """The same records in another order, with their record ids kept: the
    sampler keeps the same records and, the sums being exact, the partials
    are bit-identical."""
    n = ev.dataset("small")[0].size
    fields = ev.bound_fields(mode, "small")
    a = _oracle("small", fields)
    b = _oracle("small", fields, order=np.random.default_rng(5).permutation(n))
    for k in ("rows", "count", "sum", "nsum", "nsq"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------ the API's view
def test_per_privacy_id_with_partition_sum_bounds_is_rejected_by_the_plan():
    """AggregateParams accepts max_contributions with min/max_sum_per_partition
    and SUM, but the SUM sensitivities then have linf without l0 and
    Sensitivities raises -- as the reference's compute_sensitivities_for_sum
    (dp_computations.py:736-749) and Sensitivities.__post_init__ do.  The
    rejection stays; the matrix reaches the kernels' PER_PRIVACY_ID x
    CLIP_PARTITION branch through overridden bound fields
    (exact_values.override_plan)."""
    params = pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM], max_contributions=5,
                                 min_sum_per_partition=-1.0, max_sum_per_partition=9.0)
    with pytest.raises(ValueError, match="l0 and linf"):
        combiners.CompoundPlan(params, pdp.NaiveBudgetAccountant(1.0, 1e-6))


def _check(params):
    import torch
    eng = pdp.DPEngine(pdp.NaiveBudgetAccountant(1.0, 1e-6), pdp.MI355XBackend(device=0, seed=1))
    col = pdp.ColumnarData(pid=torch.tensor([1]), pk=torch.tensor([0]),
                           value=torch.tensor([0.5]), n_partitions=1)
    eng._check_aggregate_params(col, params, pdp.DataExtractors("pid", "pk", "value"))


def test_variance_with_max_contributions_is_rejected_by_the_engine():
    """The issue's PER_PRIVACY_ID x ItemV request (VARIANCE, MEAN, COUNT with
    max_contributions) is rejected by DPEngine, as by the reference's
    (dp_engine.py:404-414: only PRIVACY_ID_COUNT, COUNT, SUM and MEAN).  The
    rejection stays; perpid_var requests MEAN and COUNT, which run the same
    ItemV items (normalised sum and sum of squares)."""
    params = pdp.AggregateParams(metrics=[pdp.Metrics.VARIANCE, pdp.Metrics.MEAN,
                                          pdp.Metrics.COUNT], max_contributions=5,
                                 min_value=-1.0, max_value=5.0)
    with pytest.raises(NotImplementedError, match="max_contributions is not supported"):
        _check(params)


def test_every_request_passes_the_engine_checks():
    for mode, gen in ev.PAIRS:
        _check(ev.make_params(mode, gen))


@pytest.mark.parametrize("mode", sorted(ev.MODES))
def test_modes_map_to_their_cells(mode):
    _, want_mode, want_sum = ev.MODES[mode]
    f = ev.bound_fields(mode, "small")
    assert (f["mode"], f["sum_mode"]) == (want_mode, want_sum)
    # the item layout (dpg_api.hip dpg_bound_aggregate): moments without the
    # SUM bit and without per-partition clipping -> ItemV; moments with it ->
    # Item32; no moments -> Item16
    var = bool(f["metric_mask"] & (combiners.M_MEAN | combiners.M_VARIANCE))
    has_sum = bool(f["metric_mask"] & combiners.M_SUM)
    assert var == (mode in ("perpid_var", "mean_var", "item32"))
    if var:
        assert has_sum == (mode == "item32")


def test_mean_with_sum_runs_itemv_through_the_api():
    """MEAN + SUM through AggregateParams leaves the SUM bit of the metric
    mask clear: the device runs ItemV items and the engine allocates no sum
    partial.  Item32 is reached by exact_values.override_plan only."""
    plan = combiners.CompoundPlan(ev.make_params("item32", "small"),
                                  pdp.NaiveBudgetAccountant(1.0, 1e-6))
    assert plan.mask & combiners.M_MEAN and not plan.mask & combiners.M_SUM


# -------------------------------------------------------------- non-vacuity
def _widened(fields, lo=True, hi=True):
    f = dict(fields)
    a, b = (("min_sum_per_partition", "max_sum_per_partition")
            if fields["sum_mode"] == ev.CLIP_PARTITION else ("min_value", "max_value"))
    if lo:
        f[a] = -1e9
    if hi:
        f[b] = 1e9
    return f


@pytest.mark.parametrize("mode,gen", ev.PAIRS, ids=[f"{m}-{g}" for m, g in ev.PAIRS])
def test_bounds_bind(mode, gen):
    """Conditions on the inputs, by the oracle alone: sampling drops records;
    the clamp changes the sums of at least 10 % of the occupied partitions
    (`sum` is compared: the oracle accumulates it in every value mode, and
    widening a value range also moves the midpoint of nsum / nsq); under
    CLIP_PARTITION the lower and the upper sum bound each bind somewhere."""
    n = ev.dataset(gen)[0].size
    fields = ev.bound_fields(mode, gen)
    ref = _oracle(gen, fields)
    assert 0 < ref["count"].sum() < n
    if fields["sum_mode"] == ev.NONE:
        return
    occupied = ref["rows"] > 0
    free = _oracle(gen, _widened(fields))
    assert np.array_equal(free["count"], ref["count"])
    share = (free["sum"] != ref["sum"])[occupied].mean()
    assert share >= 0.10, share
    if fields["sum_mode"] == ev.CLIP_PARTITION:
        assert not np.array_equal(_oracle(gen, _widened(fields, hi=False))["sum"], ref["sum"])
        assert not np.array_equal(_oracle(gen, _widened(fields, lo=False))["sum"], ref["sum"])


def test_merge_inputs_reach_both_branches():
    """The two-level merge writes a range of 4096 partitions by plain stores
    when its kept pairs fit one tile of 65536 and by atomics when they span
    several: the uniform input has only single-tile ranges, the hot one puts
    more than a tile's pairs into range 0 -- in every mode run on them."""
    for mode in ("item32", "mean_var", "cross_sum_pp"):
        rows = _oracle("merge_uniform", ev.bound_fields(mode, "merge_uniform"))["rows"]
        pad = -rows.size % ev.MERGE_RANGE
        per_range = np.pad(rows, (0, pad)).reshape(-1, ev.MERGE_RANGE).sum(axis=1)
        assert 0 < per_range.max() <= ev.MERGE_TILE
        rows = _oracle("merge_hot", ev.bound_fields(mode, "merge_hot"))["rows"]
        assert rows[:ev.MERGE_RANGE].sum() > 2 * ev.MERGE_TILE
        assert rows[ev.MERGE_RANGE:].sum() == 0
