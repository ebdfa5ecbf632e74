#!/usr/bin/env python
"""Times the dataset histograms on one GPU, in one run:

* one_call: dpg_dataset_histograms of this tree's library;
* one_call_parent: the same call of another build of the library
  (--parent-lib: the parent commit's libdpg.so, built into a directory of its
  own) -- the call must not have become slower;
* phases: dpg_hist_pairs, dpg_hist_partitions on its own totals and
  dpg_hist_sums on its own range: what one rank of the multi-rank route runs
  on the device.  Its difference to one_call is the cost of the P-sized pass
  that writes the per-partition totals and of the three calls' overhead.

The input is a pk-sorted pre-aggregate as dpg_preaggregate leaves it (counts
1..19, about one leader in eight).  The outputs are compared first (integers,
edges and maxima bit for bit; the LINF_SUM sums, float atomics, to 1e-9).
Event timing; every candidate is warmed up, then the candidates take turns
(--runs rounds, one timed call each per round), so drift hits all alike.  One
is called slower than another only when the medians differ by more than three
times the larger run-to-run spread (max - min) of the two.  For comparison the
result quotes the split and merge times of profiles/pair_exchange.json: what
moving the pairs to their partitions' owners would have added.  Writes
profiles/hist_phases.json.

    python tools/bench_hist_phases.py [--pairs 100000000] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pipelinedp_amd import _native  # noqa: E402

NB, NS = _native.HIST_INT_BINS, _native.HIST_SUM_BINS


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


def _verdict(ms, a, b):
    """a against b: 'faster' / 'slower' only beyond three times the larger spread."""
    spread = max(max(ms[k]) - min(ms[k]) for k in (a, b))
    diff = statistics.median(ms[b]) - statistics.median(ms[a])
    if abs(diff) <= 3 * spread:
        return "not distinguishable"
    return "faster" if diff > 0 else "slower"


class _Outputs:
    def __init__(self):
        i64, f64 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.float64, device="cuda")
        self.ib = torch.empty((5, NB, 3), **i64)
        self.sc = torch.empty(NS, **i64)
        self.ss, self.sm = torch.empty(NS, **f64), torch.empty(NS, **f64)
        self.lowers = torch.empty(NS + 1, **f64)
        self.struct = _native.HistOut(self.ib.data_ptr(), self.sc.data_ptr(), self.ss.data_ptr(),
                                      self.sm.data_ptr(), self.lowers.data_ptr())

    def same_as(self, other):
        for name in ("ib", "sc", "sm", "lowers"):
            a, b = getattr(self, name), getattr(other, name)
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name
        assert torch.allclose(self.ss, other.ss, rtol=1e-9, atol=1e-9)


def _parent_call(path):
    """dpg_dataset_histograms of another build of the library, on a context
    of its own."""
    lib = ctypes.CDLL(path)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.dpg_ctx_create.argtypes = [ctypes.c_int, ctypes.c_uint64]
    lib.dpg_ctx_create.restype = vp
    lib.dpg_dataset_histograms.argtypes = [vp, vp, i64, vp, i64, i32,
                                           ctypes.POINTER(_native.HistOut), vp]
    lib.dpg_dataset_histograms.restype = ctypes.c_int
    handle = lib.dpg_ctx_create(0, 1)
    assert handle, "dpg_ctx_create of the parent library failed"

    def call(pairs_ptr, n, starts_ptr, P, out):
        st = lib.dpg_dataset_histograms(handle, pairs_ptr, n, starts_ptr, P, 0,
                                        ctypes.byref(out), None)
        assert st == 0, st
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--partitions", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_phases.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hist_phases.py needs a GPU: nothing is measured without one")
    n, P = args.pairs, args.partitions
    g = torch.Generator(device="cuda").manual_seed(1)
    pairs = torch.empty((n, 3), device="cuda", dtype=torch.float64)
    pairs[:, 1] = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 7 - 1
    words = pairs.view(torch.int32).view(-1, 6)

    def ints(lo, hi):
        return torch.randint(lo, hi, (n,), generator=g, device="cuda", dtype=torch.int32)

    pk = torch.sort(ints(0, P)).values
    words[:, 0] = pk
    words[:, 1] = ints(1, 20)                                 # records of the pair
    words[:, 4] = ints(1, 50)                                 # n_partitions
    ncl = ints(1, 200)                                        # n_contributions | leader << 31
    words[:, 5] = torch.where(ints(0, 8) == 0, ncl | -(1 << 31), ncl)
    del ncl
    starts = torch.searchsorted(pk.to(torch.int64), torch.arange(P + 1, device="cuda"))
    del pk
    torch.cuda.synchronize()

    ctx = _native.Context(0, 1)
    one, ph = _Outputs(), _Outputs()
    rows = torch.empty(P, dtype=torch.int64, device="cuda")
    count = torch.empty(P, dtype=torch.int64, device="cuda")
    rng = torch.empty(2, dtype=torch.float64, device="cuda")
    stages = {}

    def one_call():
        ctx.dataset_histograms(pairs.data_ptr(), n, starts.data_ptr(), P, False, one.struct, None)

    def phases(record=False):
        ctx.hist_pairs(pairs.data_ptr(), n, starts.data_ptr(), P, ph.ib.data_ptr(),
                       rows.data_ptr(), count.data_ptr(), rng.data_ptr(), None)
        if record:
            stages.update(ctx.stage_times())
        ctx.hist_partitions(rows.data_ptr(), count.data_ptr(), P, ph.ib.data_ptr(), None)
        if record:
            stages.update(ctx.stage_times())
        ctx.hist_sums(pairs.data_ptr(), n, rng.data_ptr(), ph.sc.data_ptr(), ph.ss.data_ptr(),
                      ph.sm.data_ptr(), ph.lowers.data_ptr(), None)
        if record:
            stages.update(ctx.stage_times())

    fns = {"one_call": one_call, "phases": phases}
    one_call()  # the first calls also load the kernels and size the workspace
    one_call()
    one_stages = ctx.stage_times()
    phases()
    phases(record=True)
    torch.cuda.synchronize()
    ph.same_as(one)
    assert int(one.sc.sum().item()) == n and int(rows.sum().item()) == n
    if args.parent_lib:
        par = _Outputs()
        call = _parent_call(args.parent_lib)
        fns["one_call_parent"] = lambda: call(pairs.data_ptr(), n, starts.data_ptr(), P,
                                              par.struct)
        fns["one_call_parent"]()
        torch.cuda.synchronize()
        par.same_as(one)

    ms = _alternate(fns, args.runs)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"pairs": n, "partitions": P, "runs": args.runs, "median_ms": med,
           "min_ms": {k: min(v) for k, v in ms.items()},
           "max_ms": {k: max(v) for k, v in ms.items()},
           "spread_ms": {k: max(v) - min(v) for k, v in ms.items()},
           "stage_ms_one_call": one_stages, "stage_ms_phases": stages,
           "phases_minus_one_call_ms": med["phases"] - med["one_call"],
           "phases_vs_one_call": _verdict(ms, "phases", "one_call"),
           "device": torch.cuda.get_device_name(0)}
    if args.parent_lib:
        res["one_call_vs_parent"] = _verdict(ms, "one_call", "one_call_parent")
        res["one_call_minus_parent_ms"] = med["one_call"] - med["one_call_parent"]
    px = os.path.join(ROOT, "profiles", "pair_exchange.json")
    if os.path.exists(px):
        with open(px) as f:
            old = json.load(f)
        if old.get("pairs") == n and old.get("partitions") == P:
            res["pair_exchange_route_ms"] = {k: old["median_ms"][k] for k in ("split", "merge")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
