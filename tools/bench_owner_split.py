#!/usr/bin/env python
"""Times the owner split of a multi-GPU release with percentiles or VECTOR_SUM
(dpg_owner_split_keys) against two yardsticks on the same tensors, in one run:

* the torch fallback: pk % R, a stable argsort, a bincount and the gathers
  of the re-based keys (and of the source positions);
* device-to-device copies sized by the bytes the split moves (every key read
  twice and written once, 24 B per key; 28 B with the source positions): one
  of a buffer of that many bytes, as tools/bench_shard.py does (the copy then
  reads and writes them, twice the split's traffic), and one of half of
  them, whose reads plus writes equal the split's traffic.

The keys are sorted tree keys pk << 16 | leaf, as dpg_quantile_keys leaves
them.  Both forms of the call (with and without out_src) alternate with the
yardsticks.  Event timing, warm-up, median of --runs.  Writes
profiles/owner_split.json.

    python tools/bench_owner_split.py [--keys 100000000] [--ranks 8] [--runs 11]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native  # noqa: E402

LOW_BITS = 16


def _time(fn, runs, warmup=2):
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
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--partitions", type=int, default=1_000_000)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "owner_split.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_owner_split.py needs a GPU: nothing is measured without one")
    n, R = args.keys, args.ranks
    g = torch.Generator(device="cuda").manual_seed(1)
    pk = torch.randint(0, args.partitions, (n,), generator=g, device="cuda", dtype=torch.int64)
    leaf = torch.randint(0, 1 << LOW_BITS, (n,), generator=g, device="cuda", dtype=torch.int64)
    keys = torch.sort((pk << LOW_BITS) | leaf).values
    del pk, leaf
    n_keys = torch.tensor([n], dtype=torch.int64, device="cuda")
    o_keys = torch.empty_like(keys)
    o_src = torch.empty(n, dtype=torch.int32, device="cuda")
    counts = torch.empty(R, dtype=torch.int64, device="cuda")
    ctx = _native.Context(0, 1)

    def split(src):
        ctx.owner_split_keys(keys.data_ptr(), n_keys.data_ptr(), n, LOW_BITS, R, o_keys.data_ptr(),
                             o_src.data_ptr() if src else None, counts.data_ptr(), None)

    t_out = {}

    def fallback(src):
        p = keys >> LOW_BITS
        dest = p % R
        order = torch.argsort(dest, stable=True)
        t_out["c"] = torch.bincount(dest, minlength=R)
        t_out["keys"] = (((p // R) << LOW_BITS) | (keys & ((1 << LOW_BITS) - 1)))[order]
        if src:
            t_out["src"] = order.to(torch.int32)

    bufs = {b: (torch.empty(b * n // 8, dtype=torch.int64, device="cuda"),
                torch.empty(b * n // 8, dtype=torch.int64, device="cuda"))
            for b in (12, 14, 24, 28)}

    # same result first: the split is the fallback's, exactly
    fallback(True)
    split(True)
    torch.cuda.synchronize()
    assert torch.equal(counts, t_out["c"]) and torch.equal(o_keys, t_out["keys"])
    assert torch.equal(o_src, t_out["src"])
    o_keys.zero_()
    split(False)
    torch.cuda.synchronize()
    assert torch.equal(o_keys, t_out["keys"])
    t_out.clear()
    split(True)
    stages = ctx.stage_times()

    fns = {"split": lambda: split(False), "split_src": lambda: split(True),
           "torch_fallback": lambda: fallback(False), "torch_fallback_src": lambda: fallback(True),
           "d2d_copy_24B": lambda: bufs[24][1].copy_(bufs[24][0]),
           "d2d_copy_28B": lambda: bufs[28][1].copy_(bufs[28][0]),
           "d2d_copy_12B": lambda: bufs[12][1].copy_(bufs[12][0]),
           "d2d_copy_14B": lambda: bufs[14][1].copy_(bufs[14][0])}
    ms = {k: [] for k in fns}
    for rep in range(2):  # alternate: two rounds of every candidate
        for k, fn in fns.items():
            ms[k] += _time(fn, (args.runs + 1) // 2)
            t_out.clear()
    med = {k: statistics.median(v) for k, v in ms.items()}
    # call -> (fallback, copy of the same bytes, copy of the same traffic, bytes per key)
    pairs = {"split": ("torch_fallback", "d2d_copy_24B", "d2d_copy_12B", 24),
             "split_src": ("torch_fallback_src", "d2d_copy_28B", "d2d_copy_14B", 28)}
    res = {"keys": n, "partitions": args.partitions, "ranks": R, "low_bits": LOW_BITS,
           "runs": {k: len(v) for k, v in ms.items()},
           "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()},
           "stage_ms_split_src": stages,
           "bytes_per_key": {k: v[3] for k, v in pairs.items()},
           "split_traffic_GBps": {k: v[3] * 1e-6 * n / med[k] for k, v in pairs.items()},
           "copy_traffic_GBps": {k: v[3] * 1e-6 * n / med[v[2]] for k, v in pairs.items()},
           "same_bytes_copy_over_split": {k: med[v[1]] / med[k] for k, v in pairs.items()},
           "same_traffic_copy_over_split": {k: med[v[2]] / med[k] for k, v in pairs.items()},
           "speedup_over_torch": {k: med[v[0]] / med[k] for k, v in pairs.items()},
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
