#!/usr/bin/env python
"""Times the device encoding of a string partition-key column (DESIGN.md
section 18): candidates on the same column in one run.

  (a) route    string_columns.encode_partition_keys end to end: hash, table
               fill, dpg_keydict_insert_slots, representatives, verify, the one
               host synchronisation, the distinct strings to the host, their
               decode and sort, dpg_keydict_gather_ids
  (b) hash, representatives, verify
               each of the three new kernels alone, on prepared inputs (the
               fill of rep is outside the timed window)
  (c) copy     a device-to-device copy of the column's offsets and bytes: what
               the hash reads, written once -- the traffic yardstick
  (d) host     columnar._encode_keys (numpy unique on an object array) on a
               --sample record sample of the same strings, host wall time,
               SCALED linearly to --records and labelled as scaled (the sort is
               n log n, so the scaling flatters the host)

The column: --records uniform draws over --keys distinct random strings of 8 to
24 bytes (printable ASCII).  Device events around each candidate, the
candidates alternating, 2 warm-up calls each, median of --runs.  No threshold is
attached: the numbers are read against (c) and (d).  Writes
profiles/string_columns.json.

    python tools/bench_string_columns.py [--records 100000000] [--keys 1000000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native, columnar, distributed, string_columns  # noqa: E402
from pipelinedp_amd.string_columns import StringColumn  # noqa: E402

WARMUP = 2
MIN_LEN, MAX_LEN = 8, 24


def _ms(fn, prep=None):
    if prep is not None:
        prep()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {"median_ms": {k: statistics.median(v) for k, v in ms.items()},
            "min_ms": {k: min(v) for k, v in ms.items()},
            "max_ms": {k: max(v) for k, v in ms.items()}}


def string_column(n, n_keys, dev):
    """n uniform draws over n_keys distinct strings of MIN_LEN..MAX_LEN bytes:
    (offsets int64 [n + 1], data uint8) on the device, and the pool as a host
    StringColumn."""
    g = torch.Generator(device=dev).manual_seed(18)
    plen = torch.randint(MIN_LEN, MAX_LEN + 1, (n_keys,), generator=g, device=dev)
    poff = torch.zeros(n_keys + 1, dtype=torch.int64, device=dev)
    torch.cumsum(plen, 0, out=poff[1:])
    pdata = torch.randint(33, 127, (int(poff[-1].item()),), generator=g, device=dev,
                          dtype=torch.uint8)
    # the first 8 bytes spell the key's number: the strings are distinct
    digits = torch.arange(n_keys, device=dev).view(-1, 1) // (10 ** torch.arange(
        7, -1, -1, device=dev)) % 10 + 48
    pdata[(poff[:-1].view(-1, 1) + torch.arange(8, device=dev)).view(-1)] = \
        digits.to(torch.uint8).view(-1)
    pick = torch.empty(n, dtype=torch.int64, device=dev)
    step = 1 << 24
    for lo in range(0, n, step):
        m = min(step, n - lo)
        pick[lo:lo + m] = torch.randint(0, n_keys, (m,), generator=g, device=dev)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(plen[pick], 0, out=offsets[1:])
    data = torch.empty(int(offsets[-1].item()), dtype=torch.uint8, device=dev)
    for lo in range(0, n, step):
        m = min(step, n - lo)
        ln = plen[pick[lo:lo + m]]
        a, b = int(offsets[lo].item()), int(offsets[lo + m].item())
        owner = torch.repeat_interleave(torch.arange(m, device=dev), ln, output_size=b - a)
        within = torch.arange(b - a, device=dev) - (offsets[lo:lo + m] - a)[owner]
        data[a:b] = pdata[poff[pick[lo:lo + m]][owner] + within]
        del owner, within
    pool = StringColumn(poff.cpu().numpy(), pdata.cpu().numpy())
    return offsets, data, pick, pool


def measure(n, n_keys, sample, runs, dev):
    offsets, data, pick, pool = string_column(n, n_keys, dev)
    col = StringColumn(offsets, data)
    ctx = _native.Context(0, 1)
    keep = {}

    def route():
        keep["ids"], keep["table"], _ = string_columns.encode_partition_keys(
            col, None, dev, ctx, n_keys)

    # the ids are right first: record i holds the string of its draw
    route()
    names = pool.to_strings()
    rank = {s: i for i, s in enumerate(keep["table"])}
    want = torch.tensor([rank.get(s, -1) for s in names], dtype=torch.int64, device=dev)[pick]
    assert torch.equal(keep["ids"], want)
    distinct = len(keep["table"])
    del want, rank
    keep.clear()

    # the host encoding of a sample of the same strings
    m = min(sample, n)
    sample_strings = [names[i] for i in pick[:m].cpu().tolist()]

    def host():
        t0 = time.perf_counter()
        columnar._encode_keys(sample_strings, torch.device("cpu"))
        return time.perf_counter() - t0

    # prepared inputs of the kernels alone
    capacity = distributed._pid_capacity(n, n_keys)
    keys, info = string_columns.device_keys(offsets, data, 0, ctx)
    slots = torch.full((capacity,), -(1 << 63), dtype=torch.int64, device=dev)
    kinfo = torch.zeros(2, dtype=torch.int64, device=dev)
    rec_slots = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.keydict_insert_slots(keys.data_ptr(), n, slots.data_ptr(), capacity,
                             rec_slots.data_ptr(), kinfo.data_ptr(), None)
    del slots
    rep = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
    ctx.keydict_representatives(rec_slots.data_ptr(), n, capacity, rep.data_ptr(), None)
    rep_timed = torch.empty_like(rep)
    mism = torch.zeros(1, dtype=torch.int64, device=dev)
    off2, data2 = torch.empty_like(offsets), torch.empty_like(data)

    def copy():
        off2.copy_(offsets)
        data2.copy_(data)

    fns = {
        "route": (route, keep.clear),
        "hash": (lambda: ctx.string_hash(offsets.data_ptr(), data.data_ptr(), data.numel(), n, 0,
                                         keys.data_ptr(), info.data_ptr(), None), None),
        "representatives": (lambda: ctx.keydict_representatives(
            rec_slots.data_ptr(), n, capacity, rep_timed.data_ptr(), None),
            lambda: rep_timed.fill_(-1)),
        "verify": (lambda: ctx.string_verify(offsets.data_ptr(), data.data_ptr(), data.numel(), n,
                                             rec_slots.data_ptr(), rep.data_ptr(),
                                             mism.data_ptr(), None), None),
        "copy": (copy, None),
    }
    host_s = []
    ms = {k: [] for k in fns}
    for i in range(WARMUP + runs):
        print(f"[bench_string_columns] round {i + 1} of {WARMUP + runs}", file=sys.stderr,
              flush=True)
        for k, (fn, prep) in fns.items():
            t = _ms(fn, prep)
            if i >= WARMUP:
                ms[k].append(t)
        t = host()
        if i >= WARMUP:
            host_s.append(t)
    assert int(info.item()) == 0 and kinfo.tolist() == [0, 0] and int(mism.item()) == 0
    assert torch.equal(rep, rep_timed)
    stats = _stats(ms)
    med = stats["median_ms"]
    host_med = statistics.median(host_s) * 1e3
    n_bytes = int(data.numel())
    res = {"records": n, "keys": n_keys, "distinct": distinct, "string_bytes": n_bytes,
           "bytes_per_string": n_bytes / max(n, 1), "table_slots": capacity,
           "runs": runs, "warmup": WARMUP, "device_events": stats,
           "host_encode_keys": {"sample_records": m, "median_ms_on_sample": host_med,
                                "scaled_to_records_ms": host_med * n / max(m, 1),
                                "scaled": True,
                                "note": "host wall time of columnar._encode_keys on the sample, "
                                        "multiplied by records / sample_records"},
           "route_over_copy": med["route"] / med["copy"],
           "hash_over_copy": med["hash"] / med["copy"],
           "verify_over_copy": med["verify"] / med["copy"],
           "scaled_host_over_route": host_med * n / max(m, 1) / med["route"]}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_columns.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_string_columns.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = measure(args.records, args.keys, args.sample, args.runs, dev)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
