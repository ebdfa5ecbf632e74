#!/usr/bin/env python
"""Times the encode of wide int64 privacy ids to dense ids in one process: four
candidates on the same column in one run.

  (a) slots    distributed.local_pid_dictionary(route="slots"): table fill,
               dpg_keydict_insert_slots, dpg_keydict_keys, the read of the
               distinct count, dpg_sort_pairs_u64, dpg_keydict_assign,
               dpg_keydict_gather_ids -- the table is probed once per record
  (b) lookup   the same dictionary composed from dpg_keydict_insert and
               dpg_keydict_lookup, which probes the table twice per record
  (c) unique   torch.unique(return_inverse=True) on the column: the encoding
               wide ids get without the flag (columnar._encode_keys)
  (d) copy     a device-to-device copy of the column: 8 bytes read and 8
               written per record, the traffic yardstick

The ids of (a), (b) and (c) are compared first.  The probing kernels are also
timed alone on a prepared table: dpg_keydict_insert_slots against
dpg_keydict_insert (the fill is outside the timed window) and
dpg_keydict_gather_ids against dpg_keydict_lookup.

With --release the run ends with the config-2-shaped release (COUNT, SUM,
PRIVACY_ID_COUNT, max_partitions_contributed=8,
max_contributions_per_partition=2, --partitions Zipf partitions) of the wide
ids with ColumnarData(wide_privacy_ids=True), against the same release with the
ranked narrow ids and their privacy_id_range given directly, in ms per step.

The ids: --records uniform draws over --ids distinct random int64 values; the
table is sized by max_distinct = --ids.  Device events around each candidate,
the candidates alternating, 2 warm-up calls each, median of --runs.  If the
device runs out of memory the shape falls back to 1e8 records over 1e6 ids and
the result says so.  Writes profiles/privacy_id_dictionary.json.

    python tools/bench_privacy_id_dictionary.py [--records 1000000000] [--ids 10000000]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native, distributed  # noqa: E402

I64_MIN = -(1 << 63)
WARMUP = 2


def _ms(fn, prep=None):
    if prep is not None:
        prep()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(fns, runs):
    """{name: [ms] * runs}: WARMUP untimed calls of every candidate, then
    `runs` rounds that time each candidate once."""
    ms = {k: [] for k in fns}
    for i in range(WARMUP + runs):
        for k, (fn, prep) in fns.items():
            t = _ms(fn, prep)
            if i >= WARMUP:
                ms[k].append(t)
    return ms


def wide_ids(n, n_ids, device):
    """n uniform draws over n_ids distinct random int64 values."""
    g = torch.Generator(device=device).manual_seed(3)
    pool = torch.unique(torch.randint(-(1 << 62), 1 << 62, (n_ids + n_ids // 8 + 64,),
                                      generator=g, device=device, dtype=torch.int64))
    pool = pool[torch.randperm(pool.numel(), generator=g, device=device)][:n_ids]
    assert pool.numel() == n_ids
    out = torch.empty(n, dtype=torch.int64, device=device)
    step = 1 << 27
    for lo in range(0, n, step):
        m = min(step, n - lo)
        out[lo:lo + m] = pool[torch.randint(0, n_ids, (m,), generator=g, device=device)]
    return out


def _stats(ms):
    return {"median_ms": {k: statistics.median(v) for k, v in ms.items()},
            "min_ms": {k: min(v) for k, v in ms.items()},
            "max_ms": {k: max(v) for k, v in ms.items()}}


def measure(n, n_ids, runs, dev):
    pid = wide_ids(n, n_ids, dev)
    ctx = _native.Context(0, 1)
    keep = {}

    def route(name):
        finish, D, n_reserved, n_lost = distributed.local_pid_dictionary(pid, ctx, None, n_ids,
                                                                         name)
        assert (n_reserved, n_lost) == (0, 0)
        keep["ids"], keep["D"] = finish(), D

    def unique():
        uniq, keep["ids"] = torch.unique(pid, return_inverse=True)
        keep["D"] = int(uniq.numel())

    # equal ids first
    unique()
    want, distinct = keep["ids"], keep["D"]
    for name in distributed.PID_DICT_ROUTES:
        route(name)
        assert keep["D"] == distinct and torch.equal(keep["ids"], want), name
    del want
    keep.clear()
    copy_dst = torch.empty_like(pid)
    fns = {"slots": (lambda: route("slots"), keep.clear),
           "lookup": (lambda: route("lookup"), keep.clear),
           "unique": (unique, keep.clear),
           "copy": (lambda: copy_dst.copy_(pid), None)}
    routes = _stats(_alternate(fns, runs))
    keep.clear()
    del copy_dst

    # the probing kernels alone, on the table the routes use
    capacity = distributed._pid_capacity(n, n_ids)
    slots = torch.empty(capacity, dtype=torch.int64, device=dev)
    slot_ids = torch.zeros(capacity, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    miss = torch.zeros(1, dtype=torch.int64, device=dev)
    rec_slots = torch.empty(n, dtype=torch.int32, device=dev)
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    fill = lambda: slots.fill_(I64_MIN)  # noqa: E731
    kernels = {
        "insert_slots": (lambda: ctx.keydict_insert_slots(
            pid.data_ptr(), n, slots.data_ptr(), capacity, rec_slots.data_ptr(),
            info.data_ptr(), None), fill),
        "insert": (lambda: ctx.keydict_insert(
            pid.data_ptr(), n, slots.data_ptr(), capacity, info.data_ptr(), None), fill),
        # both read the table of the last insert; slot_ids is all zero
        "gather_ids": (lambda: ctx.keydict_gather_ids(
            rec_slots.data_ptr(), n, slot_ids.data_ptr(), capacity, ids.data_ptr(),
            miss.data_ptr(), None), None),
        "lookup": (lambda: ctx.keydict_lookup(
            pid.data_ptr(), n, slots.data_ptr(), slot_ids.data_ptr(), capacity, ids.data_ptr(),
            miss.data_ptr(), None), None)}
    alone = _stats(_alternate(kernels, runs))
    assert info.tolist() == [0, 0] and int(miss.item()) == 0
    med = routes["median_ms"]
    res = {"records": n, "ids": n_ids, "distinct_ids": distinct, "table_slots": capacity,
           "runs": runs, "warmup": WARMUP, "routes": routes, "kernels_alone": alone,
           "slots_over_lookup": med["slots"] / med["lookup"],
           "unique_over_slots": med["unique"] / med["slots"],
           "slots_over_copy": med["slots"] / med["copy"],
           "faster_route": "slots" if med["slots"] < med["lookup"] else "lookup",
           "product_route": distributed.PID_DICT_ROUTE}
    ctx.close()
    return res, pid


def release_ms(pid, n_ids, P, steps, dev):
    """ms per step of the config-2-shaped release: wide ids with the flag
    against their ranks given as narrow ids."""
    import pipelinedp_amd as pdp
    n = pid.numel()
    g = torch.Generator(device=dev).manual_seed(5)
    w = torch.arange(1, P + 1, device=dev, dtype=torch.float64).pow_(-1.1)
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    pk = torch.empty(n, dtype=torch.int64, device=dev)
    val = torch.empty(n, dtype=torch.float64, device=dev)
    step = 1 << 27
    for lo in range(0, n, step):
        m = min(step, n - lo)
        u = torch.rand(m, generator=g, device=dev, dtype=torch.float64)
        pk[lo:lo + m] = torch.searchsorted(cdf, u).clamp_(max=P - 1)
        val[lo:lo + m] = torch.rand(m, generator=g, device=dev, dtype=torch.float64) * 10.0
    del cdf, w
    uniq, narrow = torch.unique(pid, return_inverse=True)
    D = int(uniq.numel())
    del uniq
    backend = pdp.MI355XBackend(device=0, seed=0xD1FF5EED)
    params = pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=8,
        max_contributions_per_partition=2, min_value=0.0, max_value=10.0)
    ex = pdp.DataExtractors("pid", "pk", "value")
    cols = {"wide_flag": pdp.ColumnarData(pid=pid, pk=pk, value=val, n_partitions=P,
                                          wide_privacy_ids=True, max_distinct_privacy_ids=n_ids),
            "narrow_ranked": pdp.ColumnarData(pid=narrow, pk=pk, value=val, n_partitions=P,
                                              privacy_id_range=(0, D))}
    released = [0]

    def one(col):
        acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
        res = pdp.DPEngine(acc, backend).aggregate(col, params, ex)
        acc.compute_budgets()
        res.nonce = 0xBE7C0000 + released[0]
        released[0] += 1
        return int(res.materialize().partition_ids.numel())

    out = {}
    for name, col in cols.items():
        for _ in range(WARMUP):
            one(col)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            kept = one(col)
        b.record()
        b.synchronize()
        out[name] = {"ms_per_step": a.elapsed_time(b) / steps, "kept_partitions": kept}
    out["steps"], out["partitions"] = steps, P
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000_000)
    ap.add_argument("--ids", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--release", action="store_true",
                    help="also time the config-2-shaped release with and without the flag")
    ap.add_argument("--partitions", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "privacy_id_dictionary.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_privacy_id_dictionary.py needs a GPU: nothing is measured "
                         "without one")
    dev = torch.device("cuda", 0)
    fallback = False
    try:
        res, pid = measure(args.records, args.ids, args.runs, dev)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        fallback = True
        res, pid = measure(100_000_000, 1_000_000, args.runs, dev)
    res["fell_back_to_1e8_over_1e6"] = fallback
    res["device"] = torch.cuda.get_device_name(0)
    if args.release:
        torch.cuda.empty_cache()
        res["release"] = release_ms(pid, res["ids"], args.partitions, args.steps, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
