"""The first item level reads the kept pairs out of the bounding workgroups'
regions (SrcSeg, dpg_partition.h).  k_hist and k_scatter resolve the regions
of a sub-tile once, wave-uniformly: a window of kSegK = 8 region boundaries in
scalar registers, every lane picks its region by compares, and all loads of
the sub-tile are issued together ("window").  A sub-tile that spans more
regions than the window holds is loaded by the per-lane binary search
("lookup").  DPG_DEBUG_ITEM_PATHS=1 makes the call name the paths its
sub-tiles took as zero-length stages, items.regions=window / =lookup.

Inputs are unique (privacy id, partition) pairs, four per privacy id, under
contribution bounds that do not bind, so the item count is the record count.
Sizes: 1, 2, 1023, 1024, 1025 (the workgroup size), S - 1, S, S + 1, 2 S + 1
for the item sub-tile S = items per thread x 1024, and BIG = 2e6.

Which path an input takes follows from the region layout.  The bounding
packs a small input into few workgroups: up to 1025 pairs lie in at most 8
consecutive regions, which one window covers, so the per-lane lookup cannot
be reached at those sizes and they assert only that a path was named (the
results are checked all the same).  From S - 1 pairs on the pairs are spread
over the regions of thousands of workgroups, a few items each, and a sub-tile
spans far more than 8 of them: S - 1, S, S + 1 and 2 S + 1 assert the
lookup.  At 2e6 pairs the regions are large enough for sub-tiles to fit the
window, and BIG asserts the window (3e5 pairs still took the lookup alone).
Values follow tests/exact_values.py: every partial is compared with the C
oracle's by np.array_equal.
"""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from oracle import oracle
from oracle import utility_oracle as uo
from pipelinedp_amd import analysis
from pipelinedp_amd import combiners
from tests import exact_values as ev

pytestmark = pytest.mark.gpu

M = pdp.Metrics
# item sub-tiles (dpg_api.hip bound_and_reduce: kSegIpt x 1024)
S16 = 5 * 1024   # 16-byte items
S24 = 4 * 1024   # 24- and 32-byte items
BIG = 2_000_000        # within exact_values.MAX_RECORDS
P_WIDE = 200_000       # 49 partition ranges: 6 digit bits, one LDS atomic per item
P_FEW = 5_000          # 2 ranges: wave-aggregated ranking
P_TWO = 6_000_000      # 1465 ranges: two item levels
STRIDE = 7919          # coprime to every P here: a privacy id's four keys differ

LAYOUTS = {
    # id: (AggregateParams keywords, sets the SUM bit below AggregateParams)
    "item16": (dict(metrics=[M.COUNT, M.SUM, M.PRIVACY_ID_COUNT], min_value=0.0, max_value=10.0,
                    max_contributions_per_partition=2), False),
    "itemv": (dict(metrics=[M.MEAN, M.VARIANCE, M.COUNT], min_value=-1.0, max_value=5.0,
                   max_contributions_per_partition=1), False),
    "item32": (dict(metrics=[M.MEAN, M.SUM, M.PRIVACY_ID_COUNT], min_value=0.0, max_value=10.0,
                    max_contributions_per_partition=2), True),
}

_INPUTS = {}
_REFS = {}


def _input(n, P):
    """n unique pairs: record r belongs to privacy id r // 4, partition
    r STRIDE mod P.  Cached and read-only."""
    if (n, P) not in _INPUTS:
        r = np.arange(n, dtype=np.int64)
        arrays = (r // 4, (r * STRIDE) % P, ev.exact_values(np.random.default_rng(n), n))
        for a in arrays:
            a.setflags(write=False)
        _INPUTS[(n, P)] = arrays
    return _INPUTS[(n, P)]


def _reference(n, P, fields):
    key = (n, P, tuple(sorted(fields.items())))
    if key not in _REFS:
        pid, pk, val = _input(n, P)
        ref = oracle.bound_aggregate(pid, pk, val, fields, ev.SEED)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _paths(st):
    return sorted(k.split("=")[1] for k in st if k.startswith("items.regions="))


def _run(layout, n, P, monkeypatch):
    """One noise-free release; every partial equals the oracle's.  Returns the
    stage names."""
    monkeypatch.setenv("DPG_DEBUG_ITEM_PATHS", "1")
    kw, force_sum = LAYOUTS[layout]
    pid, pk, val = _input(n, P)
    backend = pdp.MI355XBackend(device=0, seed=ev.SEED)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    res = pdp.DPEngine(acc, backend).aggregate(
        pdp.ColumnarData(pid=torch.from_numpy(pid.copy()), pk=torch.from_numpy(pk.copy()),
                         value=torch.from_numpy(val.copy()), n_partitions=P),
        pdp.AggregateParams(max_partitions_contributed=4, **kw),
        pdp.DataExtractors("pid", "pk", "value"),
        public_partitions=list(range(P)) if P <= 20_000 else None)
    if force_sum:
        res.plan.mask |= combiners.M_SUM   # Item32: see exact_values.make_params
    acc.compute_budgets()
    res.noise_enabled = False
    res.nonce = ev.NONCE
    res.materialize()
    st = backend.ctx.stage_times()
    fields = res.last_bound_fields
    var = bool(fields["metric_mask"] & (combiners.M_MEAN | combiners.M_VARIANCE))
    has_sum = bool(fields["metric_mask"] & combiners.M_SUM)
    ref = _reference(n, P, fields)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in res.last_partials.items()}
    # the bounds do not bind: every pair is kept, the item count is n
    assert int(ref["rows"].sum()) == n
    # which partials exist says which item layout ran
    assert (got["sum"] is not None) == has_sum
    assert (got["nsum"] is not None) == (got["nsq"] is not None) == var
    assert (layout == "item16") == (has_sum and not var)
    assert (layout == "item32") == (has_sum and var)
    for k in ("rows", "count", "sum", "nsum", "nsq"):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k]), k
    return st


def _check_paths(st, n):
    paths = _paths(st)
    print(f"n={n}: item region paths {paths}")
    if n <= 1025:
        assert paths
    elif n < BIG:
        assert "lookup" in paths
    else:
        assert "window" in paths


def _sizes(S):
    return [1, 2, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 1, BIG]


@pytest.mark.parametrize("n", _sizes(S16))
def test_item16_sizes(built, monkeypatch, n):
    """COUNT + SUM + PRIVACY_ID_COUNT: 16-byte items."""
    st = _run("item16", n, P_WIDE, monkeypatch)
    assert "items:scatter" in st and "items2:scatter" not in st
    _check_paths(st, n)


@pytest.mark.parametrize("n", _sizes(S24))
def test_itemv_sizes(built, monkeypatch, n):
    """MEAN + VARIANCE: 24-byte items, 4 per thread."""
    st = _run("itemv", n, P_WIDE, monkeypatch)
    assert "items:scatter" in st and "items2:scatter" not in st
    _check_paths(st, n)


@pytest.mark.parametrize("n", [2 * S24 + 1, BIG])
def test_item32(built, monkeypatch, n):
    """MEAN + SUM through the metric mask: 32-byte items."""
    _check_paths(_run("item32", n, P_WIDE, monkeypatch), n)


@pytest.mark.parametrize("n", [S16 + 1, BIG])
def test_few_ranges_wave_aggregated_ranking(built, monkeypatch, n):
    """Two partition ranges: the scatter instantiation that ranks by wave."""
    _check_paths(_run("item16", n, P_FEW, monkeypatch), n)


@pytest.mark.parametrize("n", [2 * S16 + 1, BIG])
def test_two_item_levels(built, monkeypatch, n):
    """P large enough for two item levels: the second one reads the first
    one's contiguous output (SrcItems)."""
    st = _run("item16", n, P_TWO, monkeypatch)
    assert "items:scatter" in st and "items2:scatter" in st
    _check_paths(st, n)


def test_preaggregate_pairs(built, monkeypatch):
    """The utility pre-aggregate's 24-byte pairs (ItemPA): every pair row
    equals the oracle's."""
    monkeypatch.setenv("DPG_DEBUG_ITEM_PATHS", "1")
    n, P = 2 * S24 + 1, 50_000
    pid, pk, val = _input(n, P)
    rows = list(zip(pid.tolist(), pk.tolist(), val.tolist()))
    want = uo.preaggregate(pid.tolist(), pk.tolist(), val.tolist(), None)
    ex = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0],
                            partition_extractor=lambda r: r[1], value_extractor=lambda r: r[2])
    backend = pdp.MI355XBackend(device=0, seed=7)
    got = {}
    for key, row in analysis.preaggregate(rows, backend, ex):
        got.setdefault(key, []).append(tuple(row))
    assert set(got) == set(want)
    for key, w in want.items():
        # exact values: a pair's sum is its one value
        assert sorted(got[key]) == sorted(tuple(r) for r in w), key
    _check_paths(backend.ctx.stage_times(), n)
