#!/usr/bin/env python
"""Times the encode of sparse int64 partition keys to dense ids in one process,
twice on the same tensor in one run:

* through the device key dictionary (distributed.build_key_dictionary with
  group=None: dpg_keydict_insert, dpg_keydict_keys, dpg_sort_pairs_u64,
  dpg_keydict_assign, dpg_keydict_lookup), with the table sized by the record
  count (the default) and by --max-distinct;
* through today's route, columnar._encode_keys: torch.unique with
  return_inverse over all records.

It also times dpg_keydict_insert (into a freshly filled table; the fill is
outside the timed window) and dpg_keydict_lookup alone against a
device-to-device copy of the key column (8 bytes read and 8 written per
record; the insert reads 8 and the lookup reads 8 and writes 8, both plus
their probes).

The keys: --records draws, Zipf-distributed (exponent --zipf) over --keys
distinct random int64 values.  The candidates alternate; event timing,
warm-up, median of --runs.  The ids of both routes are compared first.
Writes profiles/key_dictionary.json.

    python tools/bench_key_dictionary.py [--records 100000000] [--keys 1000000] [--runs 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native, columnar, distributed  # noqa: E402

I64_MIN = -(1 << 63)


def _time(fn, runs, warmup=2, prep=None):
    ms = []
    for i in range(warmup + runs):
        if prep is not None:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def zipf_keys(n, n_keys, exponent, device):
    """n draws from a Zipf law over n_keys distinct random int64 keys (inverse
    CDF on the device; the popular keys are scattered over the value range)."""
    g = torch.Generator(device=device).manual_seed(1)
    pool = torch.unique(torch.randint(-(1 << 61), 1 << 61, (n_keys + n_keys // 8 + 64,),
                                      generator=g, device=device, dtype=torch.int64))
    pool = pool[torch.randperm(pool.numel(), generator=g, device=device)][:n_keys]
    assert pool.numel() == n_keys
    w = torch.arange(1, n_keys + 1, device=device, dtype=torch.float64).pow_(-exponent)
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    out = torch.empty(n, dtype=torch.int64, device=device)
    step = 1 << 24
    for lo in range(0, n, step):
        u = torch.rand(min(step, n - lo), generator=g, device=device, dtype=torch.float64)
        out[lo:lo + step] = pool[torch.searchsorted(cdf, u).clamp_(max=n_keys - 1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--max-distinct", type=int, default=None,
                    help="bound of the sized table (default: 2 x --keys)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_dictionary.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_key_dictionary.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n = args.records
    max_distinct = args.max_distinct or 2 * args.keys
    pk = zipf_keys(n, args.keys, args.zipf, dev)
    ctx = _native.Context(0, 1)
    out = {}

    def dictionary(bound):
        out["kd"] = distributed.build_key_dictionary(pk, None, None, ctx, None, max_distinct=bound)

    def torch_unique():
        out["ids"], out["table"], _ = columnar._encode_keys(pk, dev)

    # same ids first: with one rank the dictionary numbers the keys as unique does
    dictionary(max_distinct)
    torch_unique()
    assert torch.equal(out["kd"].ids, out["ids"])
    distinct = int(out["kd"].n_partitions)
    assert distinct == len(out["table"])
    dictionary(None)
    assert torch.equal(out["kd"].ids, out["ids"])
    out.clear()

    # the two kernels alone, on the sized table
    capacity = max(64, 1 << (2 * max_distinct - 1).bit_length())
    slots = torch.empty(capacity, dtype=torch.int64, device=dev)
    slot_ids = torch.zeros(capacity, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    copy_dst = torch.empty_like(pk)

    def insert():
        ctx.keydict_insert(pk.data_ptr(), n, slots.data_ptr(), capacity, info.data_ptr(), None)

    def lookup():
        ctx.keydict_lookup(pk.data_ptr(), n, slots.data_ptr(), slot_ids.data_ptr(), capacity,
                           ids.data_ptr(), info.data_ptr(), None)

    fns = {"dictionary_sized": (lambda: dictionary(max_distinct), None),
           "dictionary_default": (lambda: dictionary(None), None),
           "torch_unique": (torch_unique, None),
           "keydict_insert": (insert, lambda: slots.fill_(I64_MIN)),
           "keydict_lookup": (lookup, None),  # the table of the last insert
           "d2d_copy_keys": (lambda: copy_dst.copy_(pk), None)}
    ms = {k: [] for k in fns}
    for rep in range(2):  # alternate: two rounds of every candidate
        for k, (fn, prep) in fns.items():
            ms[k] += _time(fn, (args.runs + 1) // 2, prep=prep)
            out.clear()
    assert info.tolist() == [0, 0]  # no reserved key, no overflow, no missing key
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"records": n, "keys": args.keys, "distinct_keys": distinct, "zipf": args.zipf,
           "max_distinct": max_distinct, "sized_capacity": capacity,
           "runs": {k: len(v) for k, v in ms.items()},
           "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()},
           "torch_unique_over_dictionary": {
               "sized": med["torch_unique"] / med["dictionary_sized"],
               "default": med["torch_unique"] / med["dictionary_default"]},
           "insert_over_copy": med["keydict_insert"] / med["d2d_copy_keys"],
           "lookup_over_copy": med["keydict_lookup"] / med["d2d_copy_keys"],
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
