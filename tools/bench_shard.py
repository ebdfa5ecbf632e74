#!/usr/bin/env python
"""Times the record split of the multi-GPU shuffle (dpg_shard_records) against
two yardsticks on the same tensors, in one run:

* the torch fallback: shard_of + stable argsort + three gathers;
* a device-to-device copy of the bytes the split moves (pid read twice, pk
  and value once, three columns written: 56 B per record with values).

Both forms of the scatter are timed (DPG_SHARD_STAGE=1: staged through LDS,
0: stored straight from registers), alternating with the yardsticks.  Event
timing, warm-up, median of --runs.  Writes profiles/shard_split.json.

    python tools/bench_shard.py [--records 100000000] [--ranks 8] [--runs 11]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native, distributed  # noqa: E402


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
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_split.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shard.py needs a GPU: nothing is measured without one")
    n, R = args.records, args.ranks
    g = torch.Generator(device="cuda").manual_seed(1)
    pid = torch.randint(0, 10_000_000, (n,), generator=g, device="cuda", dtype=torch.int64)
    pk = torch.randint(0, 1_000_000, (n,), generator=g, device="cuda", dtype=torch.int64)
    val = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    o_pid, o_pk, o_val = torch.empty_like(pid), torch.empty_like(pk), torch.empty_like(val)
    counts = torch.empty(R, dtype=torch.int64, device="cuda")
    ctx = _native.Context(0, 1)

    def split():
        ctx.shard_records(pid.data_ptr(), pk.data_ptr(), val.data_ptr(), n, R, o_pid.data_ptr(),
                          o_pk.data_ptr(), o_val.data_ptr(), counts.data_ptr(), None)

    def staged():
        os.environ["DPG_SHARD_STAGE"] = "1"
        split()

    def direct():
        os.environ["DPG_SHARD_STAGE"] = "0"
        split()

    t_out = {}

    def fallback():
        dest = distributed.shard_of(pid, R)
        order = torch.argsort(dest, stable=True)
        t_out["c"] = torch.bincount(dest, minlength=R)
        t_out["pid"], t_out["pk"], t_out["val"] = pid[order], pk[order], val[order]

    src = torch.empty(56 * n // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    # same result first: the split is the fallback's, exactly
    fallback()
    for fn in (staged, direct):
        fn()
        torch.cuda.synchronize()
        assert torch.equal(counts, t_out["c"]) and torch.equal(o_pid, t_out["pid"])
        assert torch.equal(o_pk, t_out["pk"]) and torch.equal(o_val, t_out["val"])
    t_out.clear()

    fns = {"split_staged": staged, "split_direct": direct, "torch_fallback": fallback,
           "d2d_copy": copy}
    ms = {k: [] for k in fns}
    for rep in range(2):  # alternate: two rounds of every candidate
        for k, fn in fns.items():
            ms[k] += _time(fn, (args.runs + 1) // 2)
            t_out.clear()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"records": n, "ranks": R, "bytes_per_record": 56, "runs": {k: len(v) for k, v in ms.items()},
           "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()},
           "copy_GBps": 56e-6 * n / med["d2d_copy"],
           "fraction_of_copy_bandwidth": {k: med["d2d_copy"] / med[k]
                                          for k in ("split_staged", "split_direct")},
           "speedup_over_torch": {k: med["torch_fallback"] / med[k]
                                  for k in ("split_staged", "split_direct")},
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
