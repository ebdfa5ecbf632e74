"""analysis.preaggregate on the GPU against the oracle's pre-aggregation
(oracle/utility_oracle.py): the rows as multisets per partition, with and
without partition sampling, the round trip through
perform_utility_analysis(pre_aggregated_data=True), and columns()."""
import collections
import functools

import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import analysis
from pipelinedp_amd import columnar
from pipelinedp_amd.analysis import utility_analysis as ua_mod
from oracle import utility_oracle as uo
from tests import ua_cases as uc

N, N_PID, P = 20_000, 500, 200
EX = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                        value_extractor=lambda r: r[2])


@functools.lru_cache(maxsize=None)
def dataset():
    """(rows, the oracle's {pk: [(count, sum, n_partitions, n_contributions)]}):
    computed once, shared, never written to."""
    rng = np.random.default_rng(91)
    pid = rng.integers(0, N_PID, N)
    w = np.arange(1, P + 1, dtype=np.float64) ** -1.1
    pk = rng.choice(P, size=N, p=w / w.sum())
    val = rng.uniform(-1, 6, N)
    rows = list(zip(pid.tolist(), pk.tolist(), val.tolist()))
    return rows, uo.preaggregate(pid.tolist(), pk.tolist(), val.tolist(), None)


def _backend():
    return pdp.MI355XBackend(device=0, seed=7)


def _assert_rows_match(got_rows, want):
    """Per partition: the same multiset of (count, n_partitions,
    n_contributions), exactly, and the sums within 1e-9 relative."""
    got = collections.defaultdict(list)
    for key, row in got_rows:
        got[key].append(tuple(row))
    assert set(got) == set(want)
    order = lambda r: (r[0], r[2], r[3], r[1])
    for key, rows in want.items():
        g, w = sorted(got[key], key=order), sorted(rows, key=order)
        assert [(r[0], r[2], r[3]) for r in g] == [(r[0], r[2], r[3]) for r in w], key
        np.testing.assert_allclose([r[1] for r in g], [r[1] for r in w], rtol=1e-9, atol=0,
                                   err_msg=str(key))


@pytest.mark.gpu
def test_rows_match_oracle(built):
    rows, want = dataset()
    got = list(analysis.preaggregate(rows, _backend(), EX))
    assert len(got) == sum(len(v) for v in want.values())
    _assert_rows_match(got, want)


@pytest.mark.gpu
def test_sampled_rows_keep_unsampled_inclusive_totals(built):
    rows, want = dataset()
    prob = 0.5
    bound = ua_mod._sample_bound(prob)
    kept = {k: v for k, v in want.items() if ua_mod._keep_by_hash(k, bound)}
    assert 0 < len(kept) < len(want)
    got = list(analysis.preaggregate(rows, _backend(), EX, partitions_sampling_prob=prob))
    # the oracle's rows carry each privacy id's totals over all partitions
    _assert_rows_match(got, kept)


@pytest.mark.gpu
def test_columns_agree_with_rows(built):
    rows, _ = dataset()
    pre = analysis.preaggregate(rows, _backend(), EX, partitions_sampling_prob=0.5)
    c = pre.columns()
    for f in ("pk", "count", "sum", "n_partitions", "n_contributions"):
        assert isinstance(c[f], torch.Tensor) and c[f].is_cuda and c[f].ndim == 1
    pk = c["pk"].cpu().numpy()
    assert (np.diff(pk) >= 0).all()                       # sorted by partition
    keys = columnar.decode_keys(pk, c["key_table"])
    from_cols = list(zip(keys, zip(c["count"].tolist(), c["sum"].tolist(),
                                   c["n_partitions"].tolist(), c["n_contributions"].tolist())))
    assert from_cols == list(pre)


@pytest.mark.gpu
def test_round_trip_through_preaggregated_analysis(built):
    rows, _ = dataset()
    params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.GAUSSIAN,
                                 metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM,
                                          pdp.Metrics.PRIVACY_ID_COUNT],
                                 max_partitions_contributed=3, max_contributions_per_partition=2,
                                 min_sum_per_partition=0.0, max_sum_per_partition=4.0)
    multi = analysis.MultiParameterConfiguration(max_partitions_contributed=[1, 3, 10],
                                                 max_contributions_per_partition=[1, 2, 5])

    def run(col, extractors, pre):
        opts = analysis.UtilityAnalysisOptions(epsilon=1.0, delta=1e-6, aggregate_params=params,
                                               multi_param_configuration=multi,
                                               pre_aggregated_data=pre)
        reports, per = analysis.perform_utility_analysis(col, _backend(), opts, extractors)
        return [uc.to_plain(r) for r in reports], {k: uc.to_plain(v) for k, v in per}

    want_rep, want_per = run(rows, EX, False)
    pre_rows = list(analysis.preaggregate(rows, _backend(), EX))
    pre_ex = pdp.PreAggregateExtractors(partition_extractor=lambda r: r[0],
                                        preaggregate_extractor=lambda r: r[1])
    got_rep, got_per = run(pre_rows, pre_ex, True)
    assert set(got_per) == set(want_per) and len(want_per) == 3 * len({r[1] for r in rows})
    for key, want in want_per.items():
        uc.assert_close(want, got_per[key], f"per{key}", atol=1e-7, rtol=1e-7)
    for want, got in zip(want_rep, got_rep):
        uc.assert_close(want, got, "report", atol=1e-7, rtol=1e-7)


class _TwoRanks(pdp.MI355XBackend):
    world_size = 2


def test_two_ranks_raise_from_host_state():
    """No device work: the backend's context is never created."""
    backend = _TwoRanks(device=0, seed=1)
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        analysis.preaggregate([(0, 0, 1.0)], backend, EX)
    assert backend._ctx is None


def test_sampling_probability_is_validated():
    with pytest.raises(ValueError, match="partitions_sampling_prob"):
        analysis.preaggregate([(0, 0, 1.0)], pdp.MI355XBackend(device=0, seed=1), EX,
                              partitions_sampling_prob=0)
