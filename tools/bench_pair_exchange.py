#!/usr/bin/env python
"""Times the two device steps of the utility analysis' pair exchange
(dpg_owner_split_pairs, dpg_merge_pair_runs) on one GPU against yardsticks on
the same tensors, in one run:

* a device-to-device copy of the pairs (24 B read and 24 B written per pair:
  the traffic of a perfect one-pass move);
* the path composed of what the library had before.  Split: the pk column
  widened to 64-bit keys, dpg_owner_split_keys with out_src, a row gather and
  the re-based pk written back.  Merge: dpg_sort_pairs_u64 of (pk, position),
  a row gather and a searchsorted for the partition starts.

The input is a pk-sorted pre-aggregate (as dpg_preaggregate leaves it); the
merge runs on the split's output, R sorted runs under local partition ids.
Event timing; every candidate is warmed up, then the candidates take turns
(--runs rounds, one timed call each per round), so drift hits all alike.  A
kernel is called faster than an alternative only when the medians differ by
more than three times the larger run-to-run spread (max - min) of the two.
Writes profiles/pair_exchange.json.

    python tools/bench_pair_exchange.py [--pairs 100000000] [--ranks 8] [--runs 12]
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


def _pk_column(pairs):
    """int32 view of the pk words of float64 [n, 3] pair entries."""
    return pairs.view(torch.int32).view(-1, 6)[:, 0]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(fns, runs):
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(_timed(fn))
    return ms


def _verdict(ms, kernel, other):
    """'faster' / 'slower' only beyond three times the larger spread."""
    spread = max(max(ms[k]) - min(ms[k]) for k in (kernel, other))
    diff = statistics.median(ms[other]) - statistics.median(ms[kernel])
    if abs(diff) <= 3 * spread:
        return "not distinguishable"
    return "faster" if diff > 0 else "slower"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--partitions", type=int, default=1_000_000)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_exchange.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_exchange.py needs a GPU: nothing is measured without one")
    n, R, P = args.pairs, args.ranks, args.partitions
    P_local = (P + R - 1) // R
    g = torch.Generator(device="cuda").manual_seed(1)
    pairs = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64)
    pk = torch.sort(torch.randint(0, P, (n,), generator=g, device="cuda", dtype=torch.int32)).values
    _pk_column(pairs).copy_(pk)
    del pk
    ctx = _native.Context(0, 1)
    i64 = dict(dtype=torch.int64, device="cuda")
    s_out = torch.empty_like(pairs)
    counts = torch.empty(R, **i64)

    def split():
        ctx.owner_split_pairs(pairs.data_ptr(), n, R, s_out.data_ptr(), counts.data_ptr(), None)

    c_out = {}
    k_out, k_src = torch.empty(n, **i64), torch.empty(n, dtype=torch.int32, device="cuda")
    n_dev = torch.tensor([n], **i64)

    def split_composed():
        keys = _pk_column(pairs).to(torch.int64)
        ctx.owner_split_keys(keys.data_ptr(), n_dev.data_ptr(), n, 0, R, k_out.data_ptr(),
                             k_src.data_ptr(), counts.data_ptr(), None)
        rows = pairs.index_select(0, k_src.to(torch.int64))
        _pk_column(rows).copy_(k_out)
        c_out["pairs"] = rows

    copy_dst = torch.empty_like(pairs)

    def copy():
        copy_dst.copy_(pairs)

    # same result first: both splits agree on every byte
    split()  # the first call also loads the kernels and sizes the workspace
    split()
    split_stages = ctx.stage_times()
    split_composed()
    torch.cuda.synchronize()
    assert torch.equal(s_out.view(torch.int64), c_out["pairs"].view(torch.int64))
    c_out.clear()
    run_start = [0] + torch.cumsum(counts, 0).tolist()

    m_out = torch.empty_like(pairs)
    starts = torch.empty(P_local + 1, **i64)
    n_bad = torch.empty(1, **i64)

    def merge():
        ctx.merge_pair_runs(s_out.data_ptr(), run_start, P_local, m_out.data_ptr(),
                            starts.data_ptr(), n_bad.data_ptr(), None)

    pos = torch.arange(n, dtype=torch.int32, device="cuda")
    sk, sv = torch.empty(n, **i64), torch.empty(n, dtype=torch.int32, device="cuda")
    ids = torch.arange(P_local + 1, **i64)
    bits = max(P_local - 1, 1).bit_length()

    def merge_composed():
        keys = _pk_column(s_out).to(torch.int64)
        ctx.sort_pairs_u64(keys.data_ptr(), pos.data_ptr(), n, 0, bits, sk.data_ptr(),
                           sv.data_ptr(), None)
        c_out["pairs"] = s_out.index_select(0, sv.to(torch.int64))
        c_out["starts"] = torch.searchsorted(sk, ids)

    merge()
    merge_composed()
    torch.cuda.synchronize()
    assert int(n_bad.item()) == 0
    assert torch.equal(m_out.view(torch.int64), c_out["pairs"].view(torch.int64))
    assert torch.equal(starts, c_out["starts"])
    c_out.clear()
    merge()
    merge_stages = ctx.stage_times()

    fns = {"split": split, "split_composed": split_composed, "merge": merge,
           "merge_composed": merge_composed, "d2d_copy": copy}
    ms = _alternate(fns, args.runs)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"pairs": n, "partitions": P, "ranks": R, "runs": args.runs,
           "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()},
           "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
           "stage_ms_split": split_stages, "stage_ms_merge": merge_stages,
           "copy_bytes_per_pair": 48,
           "copy_GBps": 48e-6 * n / med["d2d_copy"],
           "over_copy": {k: med[k] / med["d2d_copy"] for k in ("split", "merge")},
           "composed_over_kernel": {"split": med["split_composed"] / med["split"],
                                    "merge": med["merge_composed"] / med["merge"]},
           "kernel_vs_composed": {"split": _verdict(ms, "split", "split_composed"),
                                  "merge": _verdict(ms, "merge", "merge_composed")},
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
