"""dpg_string_lengths, dpg_string_pack and dpg_string_verify_runs restated from
the text of include/dpg.h over Python `bytes`, one entry at a time -- slow on
purpose, and sharing nothing with pipelinedp_amd.string_columns' numpy
restatements -- and the id rule of the global string dictionary."""
import numpy as np

from tests import string_ref

M64 = (1 << 64) - 1


def _record(offsets, data_len, n, r):
    """(start, end) of record r, or None where the header calls it invalid."""
    if not 0 <= r < n:
        return None
    a, b = int(offsets[r]), int(offsets[r + 1])
    return (a, b) if 0 <= a <= b <= data_len else None


def lengths(offsets, data_len, n, records):
    """(out_len list, invalid count)."""
    out, bad = [], 0
    for r in records:
        rec = _record(offsets, data_len, n, int(r))
        bad += rec is None
        out.append(0 if rec is None else rec[1] - rec[0])
    return out, bad


def pack(offsets, data: bytes, n, records, out_offsets, out: bytearray):
    """Writes into `out` in place; returns the invalid count."""
    bad = 0
    for j, r in enumerate(records):
        rec = _record(offsets, len(data), n, int(r))
        o0, o1 = int(out_offsets[j]), int(out_offsets[j + 1])
        if rec is None or not 0 <= o0 <= o1 <= len(out) or o1 - o0 != rec[1] - rec[0]:
            bad += 1
            continue
        out[o0:o1] = data[rec[0]:rec[1]]
    return bad


def verify_runs(keys, order, offsets, data: bytes, n_strings):
    """(head list, differences, invalid among them)."""
    head, differ, invalid = [], 0, 0
    for j in range(len(keys)):
        first = j == 0 or int(keys[j]) != int(keys[j - 1])
        head.append(1 if first else 0)
        if first:
            continue
        a = j if order is None else int(order[j])
        b = j - 1 if order is None else int(order[j - 1])
        ra = _record(offsets, len(data), n_strings, a)
        rb = _record(offsets, len(data), n_strings, b)
        if ra is None or rb is None:
            differ += 1
            invalid += 1
        elif data[ra[0]:ra[1]] != data[rb[0]:rb[1]]:
            differ += 1
    return head, differ, invalid


# ---- the ids of the global string dictionary
def owner(key_u64: int, world: int) -> int:
    """distributed.key_owner: ((fmix64(key) >> 32) * R) >> 32."""
    return ((string_ref.fmix64(key_u64) >> 32) * world) >> 32


def _signed(k: int) -> int:
    return k - (1 << 64) if k >= 1 << 63 else k


def global_ids(strings, world: int, seed: int = 0, encoding: str = "utf-8"):
    """{string: i * R + owner} for a set of strings, i the ascending signed
    rank of the string's hash among its owner's hashes; and P = R * the most
    strings any owner has (at least R)."""
    key = {s: string_ref.key(s.encode(encoding), seed) for s in set(strings)}
    ids, most = {}, 1
    for r in range(world):
        mine = sorted((s for s in key if owner(key[s], world) == r),
                      key=lambda s: _signed(key[s]))
        most = max(most, len(mine))
        for i, s in enumerate(mine):
            ids[s] = i * world + r
    return ids, world * most


def owned_strings(strings, world: int, rank: int, seed: int = 0, encoding: str = "utf-8"):
    """The strings rank `rank` owns, in owned_keys (ascending signed hash) order."""
    key = {s: string_ref.key(s.encode(encoding), seed) for s in set(strings)}
    return sorted((s for s in key if owner(key[s], world) == rank),
                  key=lambda s: _signed(key[s]))
