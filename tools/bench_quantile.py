#!/usr/bin/env python
"""Times the percentile route on one GPU next to the tuned bounding of the same
input, in one process: dpg_bound_records by stage (key kernels, every radix
pass of its three sorts, the marking scan), dpg_quantile_keys (tree keys and
their sort), dpg_quantiles (the walk), and dpg_bound_aggregate as yardstick.

Stage times come from dpg_last_stage_times (HIP events on the stream), whole
calls from torch events; warm-up, median of --runs.  A radix pass that the
device skipped (one occupied digit value) still launches its kernels, which
return at once: passes under --skip-ms count as skipped.  Writes
profiles/quantile.json.

    python tools/bench_quantile.py [--records 100000000] [--pids 1000000]
        [--partitions 100000] [--runs 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native, combiners  # noqa: E402


def _time(fn, runs, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--pids", type=int, default=1_000_000)
    ap.add_argument("--partitions", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-ms", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quantile.py needs a GPU: nothing is measured without one")
    n, U, P = args.records, args.pids, args.partitions
    g = torch.Generator(device="cuda").manual_seed(1)
    pid = torch.randint(0, U, (n,), generator=g, device="cuda", dtype=torch.int64)
    w = torch.arange(1, P + 1, dtype=torch.float64, device="cuda").pow(-1.1)  # Zipf(1.1)
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    pk = torch.empty(n, dtype=torch.int64, device="cuda")
    chunk = 1 << 25
    for s in range(0, n, chunk):
        u = torch.rand(min(chunk, n - s), dtype=torch.float64, generator=g, device="cuda")
        pk[s:s + len(u)] = torch.searchsorted(cdf, u).clamp_(max=P - 1)
    val = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 12.0 - 1.0
    ctx = _native.Context(0, 1)
    bound = _native.fill(_native.BoundParams, dict(
        mode=combiners.MODE_CROSS_AND_PER, sum_mode=combiners.SUM_CLIP_VALUE,
        metric_mask=combiners.M_COUNT | combiners.M_SUM, max_partitions_contributed=8,
        max_contributions_per_partition=2, max_contributions=0, min_value=0.0, max_value=10.0,
        min_sum_per_partition=0.0, max_sum_per_partition=0.0, n_partitions=P, pid_min=0,
        pid_count=U, rec_id_offset=0, nonce=7))
    rows, count = (torch.empty(P, dtype=torch.int64, device="cuda") for _ in range(2))
    sums = torch.empty(P, dtype=torch.float64, device="cuda")
    partials = _native.Partials(P, rows.data_ptr(), count.data_ptr(), sums.data_ptr(), None, None)
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    n_keys = torch.empty(1, dtype=torch.int64, device="cuda")
    qs = [0.5, 0.9, 0.99]
    qp = _native.fill(_native.QuantileParams, dict(
        lo=0.0, hi=10.0, noise_kind=combiners.NOISE_LAPLACE, n_quantiles=len(qs), scale=64.0,
        quantiles=qs, pk_offset=0, pk_stride=1, nonce=7))
    out = torch.empty((P, len(qs)), dtype=torch.float64, device="cuda")

    def aggregate():
        ctx.bound_aggregate(pid.data_ptr(), pk.data_ptr(), val.data_ptr(), n, bound, partials, None)

    def records():
        ctx.bound_records(pid.data_ptr(), pk.data_ptr(), n, bound, keep.data_ptr(), None)

    def tree_keys():
        ctx.quantile_keys(pk.data_ptr(), val.data_ptr(), keep.data_ptr(), n, P, qp,
                          keys.data_ptr(), n_keys.data_ptr(), None)

    def walk():
        ctx.quantiles(keys.data_ptr(), n_keys.data_ptr(), P, qp, None, out.data_ptr(), None)

    # the same kept set first: per-partition counts of the flags are the bounding's
    aggregate()
    records()
    torch.cuda.synchronize()
    flagged = torch.bincount(pk[keep.bool()], minlength=P)
    assert torch.equal(flagged, count), "dpg_bound_records disagrees with dpg_bound_aggregate"

    fns = {"bound_aggregate": aggregate, "bound_records": records, "quantile_keys": tree_keys,
           "quantiles": walk}
    ms = {k: [] for k in fns}
    stages = {"bound_records": {}, "quantile_keys": {}}
    for rep in range(2):  # alternate: two rounds of every candidate
        for k, fn in fns.items():
            ms[k] += _time(fn, (args.runs + 1) // 2)
            if k in stages:
                for name, t in ctx.stage_times().items():
                    stages[k].setdefault(name, []).append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    stage_ms = {k: {name: statistics.median(t) for name, t in v.items()} for k, v in stages.items()}
    passes = {name: t for v in stage_ms.values() for name, t in v.items() if ":pass" in name}
    ran = {name: t for name, t in passes.items() if t >= args.skip_ms}
    percentile_ms = med["bound_records"] + med["quantile_keys"] + med["quantiles"]
    res = {"records": n, "privacy_ids": U, "partitions": P, "max_partitions_contributed": 8,
           "max_contributions_per_partition": 2, "percentiles": len(qs),
           "kept_records": int(keep.sum().item()), "tree_keys": int(n_keys.item()),
           "runs": {k: len(v) for k, v in ms.items()}, "median_ms": med,
           "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()}, "stage_median_ms": stage_ms,
           "radix_passes": len(passes), "radix_passes_skipped": len(passes) - len(ran),
           "radix_pass_ms_each_run": statistics.median(ran.values()) if ran else None,
           "percentile_route_ms": percentile_ms,
           "percentile_route_over_bounding": percentile_ms / med["bound_aggregate"],
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
