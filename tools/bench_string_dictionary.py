#!/usr/bin/env python
"""Times the global string dictionary in one process
against the default one-process string route, on the column of
tools/bench_string_columns.py, candidates alternating in one run.

  (a) flagged    distributed.build_string_dictionary end to end (R = 1: hash,
                 table, representatives, verify, ids from the hashes, the
                 distinct strings packed, sorted by hash, verified in runs and
                 packed into the owned table) PLUS packing and decoding the
                 strings of --kept kept partitions
  (b) unflagged  string_columns.encode_partition_keys end to end: the
                 yardstick (profiles/string_columns.json: "route")
  (c) pack       dpg_string_pack of the distinct strings alone, on prepared
                 offsets; and `pack_copy`, a device copy of the same bytes
  (d) verify_runs  dpg_string_verify_runs alone on 2 x distinct arrivals, two
                 copies of every string, adjacent under one key
  (e) gather     string_columns._gather_strings (torch indexing, decode
                 included) of the same distinct strings: what (c) and a decode
                 of the kept strings replace on the flagged route

The column: --records uniform draws over --keys distinct random strings of 8 to
24 bytes.  Device events around each candidate, 2 warm-up calls each, median of
--runs with min and max: windows of about a millisecond ((c), (d)) are to be
read with their spread.  No threshold is attached.  Several ranks are not
measured here.  Writes profiles/string_dictionary.json.

    python tools/bench_string_dictionary.py [--records 100000000] [--keys 1000000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_string_columns import WARMUP, _ms, _stats, string_column  # noqa: E402
from pipelinedp_amd import _native, distributed, string_columns  # noqa: E402
from pipelinedp_amd.string_columns import StringColumn  # noqa: E402


def measure(n, n_keys, kept, runs, dev):
    offsets, data, pick, pool = string_column(n, n_keys, dev)
    col = StringColumn(offsets, data)
    ctx = _native.Context(0, 1)
    names = pool.to_strings()
    keep = {}

    def flagged():
        sd = distributed.build_string_dictionary(col, None, None, ctx, dev, max_distinct=n_keys)
        n_owned = sd.owned_keys.numel()
        ids = torch.arange(0, n_owned, max(1, n_owned // kept), device=dev)[:kept]
        keep["sd"], keep["kept"] = sd, sd.strings(ids)

    def unflagged():
        keep["ids"], keep["table"], _ = string_columns.encode_partition_keys(
            col, None, dev, ctx, n_keys)

    # the flagged ids are right first: a record's id leads to its own string
    flagged()
    sd = keep["sd"]
    distinct = int(sd.owned_keys.numel())
    assert sd.n_partitions == distinct and len(keep["kept"]) == min(kept, distinct)
    probe = torch.arange(0, n, max(1, n // 5000), device=dev)
    assert sd.strings(sd.ids[probe]) == [names[i] for i in pick[probe].cpu().tolist()]
    hashes = sd.owned_keys
    assert bool((hashes[1:] > hashes[:-1]).all())
    # prepared inputs of the kernels alone: the distinct strings, in table order
    t_off, t_data = sd.owned_offsets, sd.owned_data
    rec = torch.randperm(distinct, device=dev)  # gathered in no particular order
    p_off = torch.zeros(distinct + 1, dtype=torch.int64, device=dev)
    torch.cumsum((t_off[1:] - t_off[:-1])[rec], 0, out=p_off[1:])
    total = int(p_off[-1].item())
    p_out = torch.empty(total, dtype=torch.uint8, device=dev)
    p_copy = torch.empty(total, dtype=torch.uint8, device=dev)
    p_info = torch.zeros(1, dtype=torch.int64, device=dev)
    # 2 x distinct arrivals: the table twice; a key's two copies adjacent
    a_off = torch.cat([t_off, t_off[1:] + t_off[-1]])
    a_data = torch.cat([t_data, t_data])
    order = torch.stack([torch.arange(distinct, device=dev),
                         torch.arange(distinct, device=dev) + distinct], 1).view(-1)
    a_keys = hashes.repeat_interleave(2)
    a_order = order.to(torch.int32)
    head = torch.empty(2 * distinct, dtype=torch.uint8, device=dev)
    v_info = torch.zeros(2, dtype=torch.int64, device=dev)
    del sd
    keep.clear()

    fns = {
        "flagged": (flagged, keep.clear),
        "unflagged": (unflagged, keep.clear),
        "pack": (lambda: ctx.string_pack(t_off.data_ptr(), t_data.data_ptr(), t_data.numel(),
                                         distinct, rec.data_ptr(), distinct, p_off.data_ptr(),
                                         p_out.data_ptr(), total, p_info.data_ptr(), None), None),
        "pack_copy": (lambda: p_copy.copy_(p_out), None),
        "verify_runs": (lambda: ctx.string_verify_runs(
            a_keys.data_ptr(), a_order.data_ptr(), a_off.data_ptr(), a_data.data_ptr(),
            a_data.numel(), 2 * distinct, 2 * distinct, head.data_ptr(), v_info.data_ptr(),
            None), None),
        "gather": (lambda: keep.__setitem__("g", string_columns._gather_strings(
            t_off, t_data, rec, "utf-8")), keep.clear),
    }
    ms = {k: [] for k in fns}
    for i in range(WARMUP + runs):
        print(f"[bench_string_dictionary] round {i + 1} of {WARMUP + runs}", file=sys.stderr,
              flush=True)
        for k, (fn, prep) in fns.items():
            t = _ms(fn, prep)
            if i >= WARMUP:
                ms[k].append(t)
    assert int(p_info.item()) == 0 and v_info.tolist() == [0, 0]
    assert int(head.sum().item()) == distinct
    assert string_columns.decode_packed(p_off[:101], p_out[:int(p_off[100].item())]) == \
        string_columns.decode_packed(*string_columns.pack_strings(t_off, t_data, rec[:100],
                                                                  ctx)[:2])
    stats = _stats(ms)
    med = stats["median_ms"]
    res = {"records": n, "keys": n_keys, "distinct": distinct, "kept_decoded": min(kept, distinct),
           "string_bytes": int(data.numel()), "distinct_string_bytes": total,
           "verify_runs_arrivals": 2 * distinct, "runs": runs, "warmup": WARMUP, "ranks": 1,
           "device_events": stats,
           "flagged_over_unflagged": med["flagged"] / med["unflagged"],
           "pack_over_copy": med["pack"] / med["pack_copy"],
           "gather_over_pack": med["gather"] / med["pack"],
           "note": "one process on one device; several ranks are not measured"}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--kept", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_dictionary.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_string_dictionary.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = measure(args.records, args.keys, args.kept, args.runs, dev)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
