#!/usr/bin/env python
"""Times the VECTOR_SUM route on one GPU, in one process, for several vector
sizes D: dpg_vector_index (key kernel and the radix passes of its sort),
dpg_vector_sums (chunk sums and the merge of the chunk partials) and
dpg_vector_clip_noise, next to two yardsticks on the same box that alternate
with them: a device-to-device copy of the kept rows' bytes, and torch's

    torch.zeros(P, D).index_add_(0, pk[keep], value[keep])

both as written (with its two gathers) and with the gathered operands made
beforehand.  The kept set is dpg_bound_records' (computed once, not timed
here: tools/bench_quantile.py times it).

Stage times come from dpg_last_stage_times (HIP events on the stream), whole
calls from torch events; warm-up, median of --runs.  Writes
profiles/vector_sum.json.

    python tools/bench_vector.py [--records 100000000] [--pids 1000000]
        [--partitions 100000] [--sizes 4,16,64] [--runs 5]
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
    ap.add_argument("--sizes", default="4,16,64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_sum.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vector.py needs a GPU: nothing is measured without one")
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
    ctx = _native.Context(0, 1)
    bound = _native.fill(_native.BoundParams, dict(
        mode=combiners.MODE_CROSS_AND_PER, sum_mode=combiners.SUM_NONE,
        metric_mask=combiners.M_COUNT, max_partitions_contributed=8,
        max_contributions_per_partition=2, max_contributions=0, min_value=0.0, max_value=0.0,
        min_sum_per_partition=0.0, max_sum_per_partition=0.0, n_partitions=P, pid_min=0,
        pid_count=U, rec_id_offset=0, nonce=7))
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.bound_records(pid.data_ptr(), pk.data_ptr(), n, bound, keep.data_ptr(), None)
    torch.cuda.synchronize()
    del pid
    keep_b = keep.bool()
    kept = int(keep_b.sum().item())
    per_partition = torch.bincount(pk[keep_b], minlength=P)
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    n_keys = torch.empty(1, dtype=torch.int64, device="cuda")

    def index():
        ctx.vector_index(pk.data_ptr(), keep.data_ptr(), n, P, keys.data_ptr(), n_keys.data_ptr(),
                         None)

    res = {"records": n, "privacy_ids": U, "partitions": P, "max_partitions_contributed": 8,
           "max_contributions_per_partition": 2, "kept_records": kept,
           "kept_rows_per_partition": {"max": int(per_partition.max().item()),
                                       "median": float(per_partition.double().median().item())},
           "chunk_rows": _native.VSUM_CHUNK, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for D in (int(x) for x in args.sizes.split(",")):
        value = torch.empty((n, D), dtype=torch.float64, device="cuda")
        for s in range(0, n, chunk):  # integer-valued rows: every order sums them exactly
            e = min(n, s + chunk)
            value[s:e] = torch.randint(-3, 14, (e - s, D), generator=g, device="cuda",
                                       dtype=torch.int32)
        sums = torch.empty((P, D), dtype=torch.float64, device="cuda")
        out = torch.empty((P, D), dtype=torch.float64, device="cuda")
        vp = _native.fill(_native.VectorParams, dict(
            size=D, norm_kind=_native.NORM_L2, max_norm=1000.0,
            noise_kind=combiners.NOISE_LAPLACE, scale=64.0, pk_offset=0, pk_stride=1, nonce=7))
        pk_kept, rows_kept = pk[keep_b], value[keep_b]
        copy_dst = torch.empty_like(rows_kept)
        ref = [None]

        def vsums():
            ctx.vector_sums(keys.data_ptr(), n_keys.data_ptr(), value.data_ptr(), n, D, P,
                            sums.data_ptr(), None)

        def clip_noise():
            ctx.vector_clip_noise(sums.data_ptr(), P, vp, None, out.data_ptr(), None)

        def copy_kept():
            copy_dst.copy_(rows_kept)

        def index_add():
            ref[0] = torch.zeros((P, D), dtype=torch.float64, device="cuda").index_add_(
                0, pk[keep_b], value[keep_b])

        def index_add_pregathered():
            ref[0] = torch.zeros((P, D), dtype=torch.float64, device="cuda").index_add_(
                0, pk_kept, rows_kept)

        index()
        vsums()
        index_add_pregathered()
        torch.cuda.synchronize()
        assert int(n_keys.item()) == kept
        assert torch.equal(sums, ref[0]), "dpg_vector_sums disagrees with index_add_"

        fns = {"vector_index": index, "vector_sums": vsums, "vector_clip_noise": clip_noise,
               "copy_kept_rows": copy_kept, "index_add": index_add,
               "index_add_pregathered": index_add_pregathered}
        ms = {k: [] for k in fns}
        stages = {"vector_index": {}, "vector_sums": {}}
        for rep in range(2):  # alternate: two rounds of every candidate
            for k, fn in fns.items():
                ms[k] += _time(fn, (args.runs + 1) // 2)
                if k in stages:
                    for name, t in ctx.stage_times().items():
                        stages[k].setdefault(name, []).append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res["sizes"][str(D)] = {
            "kept_row_bytes": kept * D * 8,
            "runs": {k: len(v) for k, v in ms.items()}, "median_ms": med,
            "min_ms": {k: min(v) for k, v in ms.items()},
            "max_ms": {k: max(v) for k, v in ms.items()},
            "stage_median_ms": {k: {name: statistics.median(t) for name, t in v.items()}
                                for k, v in stages.items()},
            "vector_sums_over_index_add": med["vector_sums"] / med["index_add"],
            "vector_sums_over_index_add_pregathered":
                med["vector_sums"] / med["index_add_pregathered"],
            "index_plus_sums_over_index_add":
                (med["vector_index"] + med["vector_sums"]) / med["index_add"],
            "vector_sums_over_copy": med["vector_sums"] / med["copy_kept_rows"],
            "vector_sums_gbps_of_kept_rows": kept * D * 8 / med["vector_sums"] / 1e6}
        del value, rows_kept, copy_dst, pk_kept
        ref[0] = None
        torch.cuda.empty_cache()
        print(f"D={D}: " + json.dumps(res["sizes"][str(D)]["median_ms"], sort_keys=True),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
