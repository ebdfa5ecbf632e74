"""Histogram-error-estimator golden-vector generator (TEST INFRASTRUCTURE,
build container only).

Imports the read-only reference (/root/reference) with the PyDP stand-in in
tests/golden/pydp_stub_ua and records, on the seeded datasets of
gen_golden_hist.py (whose rows tests/golden/dataset_histograms.json holds
under the same case names):
  * the six histograms' bins (compute_dataset_histograms, LocalBackend);
  * histogram_error_estimator.create_error_estimator for COUNT and
    PRIVACY_ID_COUNT, Laplace and Gaussian: estimate_rmse over a grid of
    (l0, linf) with bounds between, at and beyond the ratio points (bins are
    10 wide from 1000 on, so 1005 lies between two points), and
    get_ratio_dropped_l0 / get_ratio_dropped_linf over the same bounds.
Writes tests/golden/error_estimator.json.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_estimator.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden_hist as gh  # noqa: E402  (puts the stub and the reference on sys.path)

import pipeline_dp  # noqa: E402  (the reference, read-only)
from pipeline_dp.dataset_histograms import computing_histograms as ch  # noqa: E402
from pipeline_dp.dataset_histograms import histogram_error_estimator as ee  # noqa: E402
from pipeline_dp.dataset_histograms import histograms as rh  # noqa: E402

BASE_STD = {"LAPLACE": 2.5, "GAUSSIAN": 3.75}


def bounds_of(histogram):
    """Bounds at, between and beyond the histogram's ratio points."""
    pts = [int(x) for x, _ in rh.compute_ratio_dropped(histogram)]
    top = pts[-1]
    out = {0, 1, 2, 3, 7, top - 1, top, top + 1, 2 * top + 5}
    out.update(pts[1:6])
    out.update(p for p in pts if p >= 1000)
    out.update(p + 5 for p in pts[:-1] if p >= 1000)   # strictly between two points
    out.update((a + b) // 2 for a, b in zip(pts, pts[1:]) if b - a > 1)
    return sorted(b for b in out if b >= 0)


def run_case(name, seed, n, n_pid, n_pk, heavy=False):
    pid, pk, val = gh.dataset(seed, n, n_pid, n_pk, heavy)
    rows = list(zip(pid.tolist(), pk.tolist(), val.tolist()))
    ex = pipeline_dp.DataExtractors(privacy_id_extractor=lambda r: r[0],
                                    partition_extractor=lambda r: r[1],
                                    value_extractor=lambda r: r[2])
    (hs,) = list(ch.compute_dataset_histograms(rows, ex, pipeline_dp.LocalBackend()))
    l0s = bounds_of(hs.l0_contributions_histogram)
    linfs = bounds_of(hs.linf_contributions_histogram)
    # a grid that stays small: every l0 with a few linf, every linf with a few l0
    few = lambda xs: sorted(set(xs[1:4] + xs[-3:] + xs[len(xs) // 2:len(xs) // 2 + 2]))
    grid = sorted({(a, b) for a in l0s for b in few(linfs)} |
                  {(a, b) for a in few(l0s) for b in linfs})
    estimators = []
    for metric in ("COUNT", "PRIVACY_ID_COUNT"):
        for noise in ("LAPLACE", "GAUSSIAN"):
            est = ee.create_error_estimator(hs, BASE_STD[noise], pipeline_dp.Metrics.__dict__[metric],
                                            pipeline_dp.NoiseKind[noise])
            if metric == "COUNT":
                rmse = [[a, b, float(est.estimate_rmse(a, b))] for a, b in grid if a > 0]
            else:
                rmse = [[a, None, float(est.estimate_rmse(a))] for a in l0s if a > 0]
                # linf is ignored for PRIVACY_ID_COUNT
                rmse += [[a, 3, float(est.estimate_rmse(a, 3))] for a in few(l0s) if a > 0]
            estimators.append(dict(
                metric=metric, noise=noise, base_std=BASE_STD[noise], rmse=rmse,
                ratio_dropped_l0=[[a, float(est.get_ratio_dropped_l0(a))] for a in l0s],
                ratio_dropped_linf=[[b, float(est.get_ratio_dropped_linf(b))] for b in linfs]))
    return dict(name=name, histograms=gh.plain_all(hs), estimators=estimators)


def main():
    cases = [run_case("zipf_small", 11, 3000, 200, 80),
             run_case("heavy_ids", 12, 12000, 300, 1500, heavy=True)]
    path = os.path.join(HERE, "error_estimator.json")
    with open(path, "w") as f:
        json.dump(cases, f)
    print("wrote", len(cases), "estimator cases,", os.path.getsize(path), "bytes,",
          sum(len(e["rmse"]) for c in cases for e in c["estimators"]), "rmse points")


if __name__ == "__main__":
    main()
