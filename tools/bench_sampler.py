#!/usr/bin/env python
"""Times the utility analysis' partition sampler (dpg_sample_partitions)
against the host route it replaces for integer keys, in one process:

* device time of the call for dense ids at P = 1e6, 1e7, 1e8 and for a
  1e7-entry random int64 key table: device events around a window of
  back-to-back calls sized to last --window seconds, a warm-up, the median
  of --runs windows, reported per call;
* the host route on the same machine at P = 1e6 and 1e7: columnar.decode_keys
  plus the _keep_by_hash loop, the bool array, packbits and the upload
  (wall clock), and a check that both routes give the same mask;
* the time from the entry of perform_utility_analysis' analysis object to
  the end of its mask step at P = 1e7 over --records records, by the host
  route (pre_aggregation.integer_keys patched to refuse) and by the device
  route.

Writes profiles/partition_sampler.json.

    python tools/bench_sampler.py [--runs 11] [--window 1.0]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pipelinedp_amd as pdp  # noqa: E402
from pipelinedp_amd import analysis, columnar, pre_aggregation  # noqa: E402
from pipelinedp_amd.analysis import utility_analysis as ua  # noqa: E402

PROB = 0.1


def device_ms(backend, n, keys, runs, window_s):
    """Median / min / max device milliseconds per call and the repeats per window."""
    dev = backend.device
    bound = ua._sample_bound(PROB)
    mask = torch.empty(8 * ((n + 63) // 64), dtype=torch.uint8, device=dev)
    sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kp = ctypes.c_void_p(keys.data_ptr()) if keys is not None else None
    mp = ctypes.c_void_p(mask.data_ptr())

    def window(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            backend.ctx.sample_partitions(kp, 0, 1, n, bound, mp, None, sptr)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    window(3)                                            # warm-up
    repeats = max(3, int(window_s * 1e3 / (window(10) / 10)) + 1)
    window(repeats)
    ms = [window(repeats) / repeats for _ in range(runs)]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                repeats_per_window=repeats, runs=runs,
                window_ms=statistics.median(ms) * repeats), mask


def host_route(P, dev):
    """The host route of UtilityAnalysis._sample_mask, timed in its parts."""
    bound = ua._sample_bound(PROB)
    t0 = time.perf_counter()
    keys = columnar.decode_keys(np.arange(P), None)
    t1 = time.perf_counter()
    keep = np.array([ua._keep_by_hash(k, bound) for k in keys], bool)
    t2 = time.perf_counter()
    mask = torch.from_numpy(np.packbits(keep, bitorder="little")).to(dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dict(decode_keys_ms=(t1 - t0) * 1e3, keep_by_hash_loop_ms=(t2 - t1) * 1e3,
                pack_upload_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3), mask


def entry_to_mask_ms(backend, cols, device_route: bool):
    """Wall milliseconds from the analysis object's construction to the
    finished mask (pre-aggregation included), and the mask."""
    params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                 max_partitions_contributed=2, max_contributions_per_partition=1)
    opts = analysis.UtilityAnalysisOptions(epsilon=1.0, delta=1e-6, aggregate_params=params,
                                           partitions_sampling_prob=PROB)
    real = pre_aggregation.integer_keys
    if not device_route:
        pre_aggregation.integer_keys = lambda key_table: False
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run = analysis.UtilityAnalysis(cols, backend, opts, pdp.DataExtractors("pid", "pk", None))
        dev = backend.device
        _, _, P, key_table, _ = run._pairs(dev)
        t1 = time.perf_counter()
        mask = run._sample_mask(P, key_table, dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    finally:
        pre_aggregation.integer_keys = real
    return dict(total_ms=(t2 - t0) * 1e3, preaggregate_ms=(t1 - t0) * 1e3,
                mask_step_ms=(t2 - t1) * 1e3), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_sampler.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler.py needs a GPU: nothing is measured without one")
    backend = pdp.MI355XBackend(device=0, seed=7)
    dev = backend.device
    res = {"device": torch.cuda.get_device_name(0), "sampling_prob": PROB, "device_route": {},
           "host_route": {}, "host_over_device": {}}
    masks = {}
    for P in (1_000_000, 10_000_000, 100_000_000):
        res["device_route"][f"dense_{P}"], masks[P] = device_ms(backend, P, None, args.runs,
                                                                args.window)
        print("device dense", P, res["device_route"][f"dense_{P}"], flush=True)
    rng = np.random.default_rng(5)
    table = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, 10_000_000)).to(dev)
    res["device_route"]["key_table_10000000"], _ = device_ms(backend, table.numel(), table,
                                                             args.runs, args.window)
    print("device key table", res["device_route"]["key_table_10000000"], flush=True)
    del table
    res["stage_ms_last_call"] = backend.ctx.stage_times()
    for P in (1_000_000, 10_000_000):
        res["host_route"][f"dense_{P}"], hmask = host_route(P, dev)
        print("host dense", P, res["host_route"][f"dense_{P}"], flush=True)
        assert torch.equal(hmask, masks[P][:hmask.numel()]), "host and device masks differ"
        assert not masks[P][hmask.numel():].any()
        res["host_over_device"][f"dense_{P}"] = (res["host_route"][f"dense_{P}"]["total_ms"] /
                                                 res["device_route"][f"dense_{P}"]["median_ms"])
    res["masks_equal"] = True

    P = 10_000_000
    pid = torch.from_numpy(rng.integers(0, 200_000, args.records)).to(dev)
    pk = torch.from_numpy(rng.integers(0, P, args.records)).to(dev)
    cols = pdp.ColumnarData(pid=pid, pk=pk, n_partitions=P)
    entry_to_mask_ms(backend, cols, True)                          # warm-up of both stages
    after, m_after = entry_to_mask_ms(backend, cols, True)
    before, m_before = entry_to_mask_ms(backend, cols, False)
    assert torch.equal(m_before, m_after[:m_before.numel()])
    res["entry_to_mask_P1e7"] = dict(records=args.records, before_host_route=before,
                                     after_device_route=after,
                                     ratio=before["total_ms"] / after["total_ms"])
    print("entry to mask", res["entry_to_mask_P1e7"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res["host_over_device"]))
    if res["host_over_device"]["dense_10000000"] <= 1:
        raise SystemExit("the device route is not faster than the host route at P = 1e7")


if __name__ == "__main__":
    main()
