"""dataset_histograms.histogram_error_estimator against the reference's
outputs (tests/golden/error_estimator.json, written by
tests/golden/gen_golden_estimator.py from the reference itself): on the host
from the fixture's bins, and on the GPU from compute_dataset_histograms over
the same rows (tests/golden/dataset_histograms.json holds them)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import dataset_histograms
from pipelinedp_amd.dataset_histograms import histogram_error_estimator as ee
from pipelinedp_amd.dataset_histograms import histograms as hist

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "error_estimator.json")))
T = hist.HistogramType
REL = 1e-12


def fixture_histograms(case) -> hist.DatasetHistograms:
    hs = [hist.Histogram(T(h["name"]), [hist.FrequencyBin(*b) for b in h["bins"]])
          for h in case["histograms"]]
    return hist.DatasetHistograms(*hs)


def check(histograms, case):
    points = 0
    for e in case["estimators"]:
        est = ee.create_error_estimator(histograms, e["base_std"], pdp.Metrics.__dict__[e["metric"]],
                                        pdp.NoiseKind[e["noise"]])
        tag = (case["name"], e["metric"], e["noise"])
        for l0, linf, want in e["rmse"]:
            got = est.estimate_rmse(l0) if linf is None else est.estimate_rmse(l0, linf)
            assert got == pytest.approx(want, rel=REL, abs=0), (tag, l0, linf)
            points += 1
        for b, want in e["ratio_dropped_l0"]:
            assert est.get_ratio_dropped_l0(b) == pytest.approx(want, rel=REL, abs=0), (tag, b)
        for b, want in e["ratio_dropped_linf"]:
            assert est.get_ratio_dropped_linf(b) == pytest.approx(want, rel=REL, abs=0), (tag, b)
    assert points > 100


def test_module_is_exposed():
    assert dataset_histograms.histogram_error_estimator is ee


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_matches_reference_from_fixture_bins(case):
    check(fixture_histograms(case), case)


def test_fixture_covers_between_at_and_beyond():
    """The grid holds bounds at a ratio point, strictly between two points
    (interpolated) and past the last one, for l0 and linf."""
    by_name = {c["name"]: c for c in CASES}
    # (heavy_ids' LINF points are consecutive integers: nothing lies between)
    for name, attr, field in (("heavy_ids", "l0_contributions_histogram", "ratio_dropped_l0"),
                              ("zipf_small", "l0_contributions_histogram", "ratio_dropped_l0"),
                              ("zipf_small", "linf_contributions_histogram",
                               "ratio_dropped_linf")):
        case = by_name[name]
        pts = [x for x, _ in hist.compute_ratio_dropped(getattr(fixture_histograms(case), attr))]
        bounds = [b for b, _ in case["estimators"][0][field]]
        assert any(b in pts and b > 0 for b in bounds)
        assert any(pts[0] < b < pts[-1] and b not in pts for b in bounds)
        assert any(b > pts[-1] for b in bounds) and 0 in bounds


def test_count_needs_linf_and_other_metrics_raise():
    hs = fixture_histograms(CASES[0])
    est = ee.create_error_estimator(hs, 1.0, pdp.Metrics.COUNT, pdp.NoiseKind.LAPLACE)
    with pytest.raises(ValueError, match="linf"):
        est.estimate_rmse(2)
    with pytest.raises(ValueError, match="COUNT and PRIVACY_ID_COUNT"):
        ee.create_error_estimator(hs, 1.0, pdp.Metrics.SUM, pdp.NoiseKind.LAPLACE)


@functools.lru_cache(maxsize=None)
def _rows(name):
    path = os.path.join(HERE, "golden", "dataset_histograms.json")
    case = next(c for c in json.load(open(path)) if c["name"] == name)
    return case["pid"], case["pk"], case["value"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gpu_histograms_give_the_same_estimates(built, case):
    from pipelinedp_amd.dataset_histograms import computing_histograms as ch
    pid, pk, val = _rows(case["name"])
    cols = pdp.ColumnarData(pid=torch.as_tensor(np.asarray(pid, np.int64)),
                            pk=torch.as_tensor(np.asarray(pk, np.int64)),
                            value=torch.as_tensor(np.asarray(val, np.float64)))
    (hs,) = list(ch.compute_dataset_histograms(cols, pdp.DataExtractors("pid", "pk", "value"),
                                               pdp.MI355XBackend(device=0, seed=7)))
    check(hs, case)
