"""String key columns: hashed, verified and dictionary-encoded on the device.

`StringColumn` is Arrow's variable-width layout -- `offsets` (n + 1 integers)
and `data` (uint8 bytes); record i is data[offsets[i]:offsets[i + 1]] -- and is
accepted as `pid` and as `pk` of a ColumnarData.  Lists and arrays of `str`
keep the host encoding (columnar._encode_keys).

The device turns every record into a 64-bit key (dpg_string_hash; the
definition is in include/dpg.h and restated here in numpy, `host_keys`).

* A partition-key column goes through the write-once hash table of the sparse
  integer keys (`encode_partition_keys`): insert, one representative record
  per slot, and a byte compare of every record with its slot's representative,
  so a hash collision raises instead of merging two partitions.  Only the D
  distinct strings reach the host, where they are decoded and sorted.
* With ColumnarData(global_string_keys=True) a partition-key column gets its
  ids from the hashes instead (`encode_global_partition_keys`,
  distributed.build_string_dictionary), on one rank or
  several: the distinct strings are packed on the device (`pack_strings`), sent
  to their hashes' owners and compared there run by run (`verify_runs`), and
  only the strings of kept partitions are decoded (`decode_packed`).
* A privacy-id column is replaced by its keys and takes the wide-id route
  (distributed.encode_privacy_ids).  These hashes are not verified: a
  collision merges two privacy ids into one, which only makes contribution
  bounding stricter and never weakens the guarantee; no privacy id reaches a
  result; and for D distinct ids the probability of any collision is at most
  D^2 / 2^65.

DESIGN.md section 18.
"""
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

_M64 = (1 << 64) - 1
_I64_MIN = -(1 << 63)
_LEN_MUL = 0x9E3779B97F4A7C15
_KEY_EMPTY = 1 << 63  # DPG_KEYDICT_EMPTY


def _is_integer(x) -> bool:
    if isinstance(x, torch.Tensor):
        return not x.is_floating_point() and not x.is_complex() and x.dtype != torch.bool
    return x.dtype.kind in "iu"


class StringColumn:
    """A column of n strings in Arrow's variable-width layout.

    `offsets`: a 1-D integer tensor or array of n + 1 entries, ascending, with
    0 <= offsets[i] <= len(data); `data`: a 1-D uint8 tensor or array.  Record
    i is the bytes data[offsets[i]:offsets[i + 1]].  Either may be a strided or
    offset view on any device: the encoder makes them contiguous device
    tensors and copies only when they are not already.  `offsets` of another
    integer width (Arrow's int32 offsets) are widened to int64 by a copy.

    `hash_seed`: seed of the 64-bit string hash.  Two different partition
    strings that share a hash make the call raise ValueError; another seed
    separates them.

    Construction checks types and shapes on the host only (TypeError for
    offsets that are not 1-D integers or data that is not 1-D uint8, ValueError
    for fewer than one offset); the offsets' values are checked on the device
    when the column is encoded."""

    def __init__(self, offsets, data, hash_seed: int = 0, encoding: str = "utf-8"):
        if not isinstance(offsets, torch.Tensor):
            offsets = np.asarray(offsets)
        if not isinstance(data, torch.Tensor):
            data = np.asarray(data)
        if offsets.ndim != 1 or not _is_integer(offsets):
            raise TypeError("StringColumn offsets must be a 1-D integer tensor or array")
        is_u8 = data.dtype == (torch.uint8 if isinstance(data, torch.Tensor) else np.uint8)
        if data.ndim != 1 or not is_u8:
            raise TypeError("StringColumn data must be a 1-D uint8 tensor or array")
        if offsets.shape[0] < 1:
            raise ValueError("StringColumn offsets must hold n + 1 >= 1 entries")
        self.offsets = offsets
        self.data = data
        self.hash_seed = int(hash_seed)
        self.encoding = encoding

    def __len__(self) -> int:
        return int(self.offsets.shape[0]) - 1

    def __repr__(self) -> str:
        return f"StringColumn(n={len(self)}, bytes={int(self.data.shape[0])})"

    @classmethod
    def from_strings(cls, seq: Sequence[str], encoding: str = "utf-8",
                     hash_seed: int = 0) -> "StringColumn":
        """A host column holding the strings of `seq`, encoded with `encoding`."""
        raw = [s.encode(encoding) for s in seq]
        offsets = np.zeros(len(raw) + 1, dtype=np.int64)
        if raw:
            np.cumsum([len(b) for b in raw], out=offsets[1:])
        data = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
        return cls(offsets, data, hash_seed=hash_seed, encoding=encoding)

    def to_strings(self) -> List[str]:
        """The column as a list of str (tests and small inputs: a host loop)."""
        offsets, data = self.host_columns()
        buf = data.tobytes()
        off = offsets.tolist()
        if any(not 0 <= a <= b <= len(buf) for a, b in zip(off[:-1], off[1:])):
            raise ValueError("StringColumn offsets are not ascending within the data")
        return [buf[a:b].decode(self.encoding) for a, b in zip(off[:-1], off[1:])]

    def host_columns(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets int64, data uint8) as contiguous numpy arrays."""
        def host(x, dtype):
            if isinstance(x, torch.Tensor):
                x = x.detach().cpu().numpy()
            return np.ascontiguousarray(x, dtype=dtype)
        return host(self.offsets, np.int64), host(self.data, np.uint8)

    def device_columns(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(offsets int64, data uint8) as contiguous tensors on `device`,
        copied only when they are not that already."""
        def dev(x, dtype):
            if not isinstance(x, torch.Tensor):
                x = torch.from_numpy(np.ascontiguousarray(x))
            return x.to(device=device, dtype=dtype).contiguous()
        return dev(self.offsets, torch.int64), dev(self.data, torch.uint8)

    def is_on_device(self) -> bool:
        return (isinstance(self.offsets, torch.Tensor) and self.offsets.is_cuda
                and isinstance(self.data, torch.Tensor) and self.data.is_cuda)


def _fmix64(k: np.ndarray) -> np.ndarray:
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)  # uint64 products wrap
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> np.uint64(33))


def host_keys(offsets: np.ndarray, data: np.ndarray, seed: int = 0) -> Tuple[np.ndarray, int]:
    """dpg_string_hash in numpy: (int64 keys, number of records with invalid
    offsets, whose key is 0).  One vector step per word position, over the
    records that are at least that long."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    start, end = offsets[:-1], offsets[1:]
    ok = (start >= 0) & (start <= end) & (end <= data.size)
    length = np.where(ok, end - start, 0).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _fmix64(np.uint64(seed & _M64) ^ (length * np.uint64(_LEN_MUL)))
        padded = np.concatenate([data, np.zeros(8, dtype=np.uint8)])
        byte = np.arange(8, dtype=np.int64)
        words = (length + np.uint64(7)) >> np.uint64(3)
        live = np.nonzero(words > 0)[0]
        k = 0
        while live.size:
            pos = np.where(ok[live], start[live], 0)[:, None] + 8 * k + byte
            inside = (8 * k + byte)[None, :] < length[live].astype(np.int64)[:, None]
            b = np.where(inside, padded[np.minimum(pos, data.size)], 0).astype(np.uint64)
            w = (b << (np.uint64(8) * byte.astype(np.uint64))).sum(axis=1, dtype=np.uint64)
            h[live] = _fmix64(h[live] ^ w)
            k += 1
            live = live[words[live] > k]
    h[h == np.uint64(_KEY_EMPTY)] = np.uint64(_KEY_EMPTY ^ 1)
    h[~ok] = 0
    return h.view(np.int64), int((~ok).sum())


def device_keys(offsets: torch.Tensor, data: torch.Tensor, seed: int, ctx,
                stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The one place the encoders obtain string hashes: (int64 keys [n],
    int64 [1] count of records with invalid offsets) on the device, from
    contiguous device columns.  Stream-ordered, no host synchronisation."""
    dev = offsets.device
    n = offsets.numel() - 1
    if n >= 1 << 31:
        raise ValueError("a string column holds 2^31 or more records; a device takes fewer")
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ctx.string_hash(offsets.data_ptr(), data.data_ptr(), data.numel(), n, seed,
                        keys.data_ptr(), info.data_ptr(), stream)
    return keys, info


def _gather_strings(offsets, data, records: torch.Tensor, encoding: str) -> List[str]:
    """The strings of the given records (a device index tensor, D entries),
    gathered on the device and decoded on the host."""
    D = records.numel()
    if D == 0:
        return []
    start = offsets[records]
    length = offsets[records + 1] - start
    first = torch.cumsum(length, 0) - length  # where each string starts in the gathered bytes
    total = int(length.sum().item())
    owner = torch.repeat_interleave(torch.arange(D, device=records.device), length,
                                    output_size=total)
    pos = torch.arange(total, device=records.device) - first[owner] + start[owner]
    buf = data[pos].cpu().numpy().tobytes()
    a = first.tolist()
    ln = length.tolist()
    return [buf[a[i]:a[i] + ln[i]].decode(encoding) for i in range(D)]


def _np_ranges(offsets: np.ndarray, data_len: int, n: int, records: np.ndarray):
    """(start, length, valid) of the given records of an n-record host column,
    checked as the device checks them; an invalid record has length 0."""
    records = np.asarray(records, dtype=np.int64)
    ok = (records >= 0) & (records < n)
    r = np.where(ok, records, 0)
    if n == 0:
        z = np.zeros(records.shape, dtype=np.int64)
        return z, z.copy(), np.zeros(records.shape, dtype=bool)
    start, end = offsets[r], offsets[r + 1]
    ok &= (start >= 0) & (start <= end) & (end <= data_len)
    return np.where(ok, start, 0), np.where(ok, end - start, 0), ok


def host_pack(offsets: np.ndarray, data: np.ndarray, records: np.ndarray):
    """dpg_string_lengths + prefix sum + dpg_string_pack in numpy: (out_offsets
    int64[m + 1], out_data uint8, number of invalid records, which get an empty
    range)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    start, length, ok = _np_ranges(offsets, data.size, offsets.size - 1, records)
    out_offsets = np.zeros(length.size + 1, dtype=np.int64)
    np.cumsum(length, out=out_offsets[1:])
    total = int(out_offsets[-1])
    which = np.repeat(np.arange(length.size), length)
    pos = np.arange(total, dtype=np.int64) - out_offsets[:-1][which] + start[which]
    return out_offsets, data[pos], int((~ok).sum())


def host_verify_runs(keys: np.ndarray, order: Optional[np.ndarray], offsets: np.ndarray,
                     data: np.ndarray):
    """dpg_string_verify_runs in numpy: (head uint8[m], differences, of which
    invalid indices or offsets)."""
    keys = np.asarray(keys)
    m = keys.size
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    head = np.ones(m, dtype=np.uint8)
    if m > 1:
        head[1:] = keys[1:] != keys[:-1]
    idx = np.arange(m, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    start, length, ok = _np_ranges(offsets, data.size, offsets.size - 1, idx)
    buf = data.tobytes()
    differ = invalid = 0
    for j in np.nonzero(head == 0)[0].tolist():
        if not (ok[j] and ok[j - 1]):
            differ += 1
            invalid += 1
        elif (buf[start[j]:start[j] + length[j]]
              != buf[start[j - 1]:start[j - 1] + length[j - 1]]):
            differ += 1
    return head, differ, invalid


def pack_strings(offsets: torch.Tensor, data: torch.Tensor, records: torch.Tensor, ctx=None,
                 stream=None):
    """The given records (an int64 index tensor, m entries, any order, repeats
    allowed) of a column as a packed column of their own: (out_offsets
    int64[m + 1], out_data uint8, int64[1] count of invalid records), on the
    column's device.  Device tensors with the library context `ctx`:
    dpg_string_lengths, a cumsum over m entries, ONE host synchronisation that
    reads the byte total (the output must be allocated) and dpg_string_pack.
    Host tensors: the numpy restatement (`host_pack`)."""
    dev = offsets.device
    n, m = offsets.numel() - 1, records.numel()
    if ctx is None or dev.type != "cuda":
        oo, od, bad = host_pack(offsets.numpy(), data.numpy(), records.numpy())
        return torch.from_numpy(oo), torch.from_numpy(od), torch.tensor([bad], dtype=torch.int64)
    records = records.to(torch.int64).contiguous()
    with torch.cuda.device(dev):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        out_offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        info = torch.zeros(2, dtype=torch.int64, device=dev)
        ctx.string_lengths(offsets.data_ptr(), data.numel(), n, records.data_ptr(), m,
                           out_offsets.data_ptr() + 8, info.data_ptr(), stream)
        if m:
            torch.cumsum(out_offsets[1:], 0, out=out_offsets[1:])
        total = int(out_offsets[-1].item())  # the one host synchronisation
        out_data = torch.empty(total, dtype=torch.uint8, device=dev)
        # an invalid record is counted once, by the lengths: its empty out
        # range makes the pack count it again, into a slot nobody reads
        ctx.string_pack(offsets.data_ptr(), data.data_ptr(), data.numel(), n, records.data_ptr(),
                        m, out_offsets.data_ptr(), out_data.data_ptr(), total,
                        info.data_ptr() + 8, stream)
    return out_offsets, out_data, info[:1]


def verify_runs(keys: torch.Tensor, order: Optional[torch.Tensor], offsets: torch.Tensor,
                data: torch.Tensor, ctx=None, stream=None):
    """dpg_string_verify_runs over a column: (head uint8[m], int64[2] counts of
    differences and of invalid entries among them) on the keys' device; host
    tensors take the numpy restatement (`host_verify_runs`).  `order`: int32
    tensor of uint32 bit patterns, or None."""
    dev = keys.device
    m = keys.numel()
    if ctx is None or dev.type != "cuda":
        head, differ, invalid = host_verify_runs(
            keys.numpy(), None if order is None else order.numpy().view(np.uint32),
            offsets.numpy(), data.numpy())
        return torch.from_numpy(head), torch.tensor([differ, invalid], dtype=torch.int64)
    head = torch.empty(m, dtype=torch.uint8, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ctx.string_verify_runs(keys.data_ptr(), None if order is None else order.data_ptr(),
                               offsets.data_ptr(), data.data_ptr(), data.numel(),
                               offsets.numel() - 1, m, head.data_ptr(), info.data_ptr(), stream)
    return head, info


def decode_packed(out_offsets, out_data, encoding: str = "utf-8") -> List[str]:
    """A packed column (tensors on any device) as a list of str."""
    off = out_offsets.cpu().tolist()
    buf = out_data.cpu().numpy().tobytes()
    return [buf[a:b].decode(encoding) for a, b in zip(off[:-1], off[1:])]


def public_strings(public_partitions) -> Optional[List[str]]:
    """Public partitions of a string partition column as a list of str: a
    list or tuple of str, or a StringColumn; else TypeError."""
    if public_partitions is None:
        return None
    if isinstance(public_partitions, StringColumn):
        return public_partitions.to_strings()
    if isinstance(public_partitions, (list, tuple)) and all(
            isinstance(k, str) for k in public_partitions):
        return list(public_partitions)
    raise TypeError("a StringColumn of partition keys needs public partitions that are a list "
                    "or tuple of str, or a StringColumn")


def encode_partition_keys(column: StringColumn, public: Optional[List[str]], device, ctx,
                          max_distinct: Optional[int] = None):
    """Dense partition ids of a string column, one process: returns (ids int64
    [n] on the device, the key table -- the sorted list of the distinct
    strings, public ones included --, the ids of `public` as an int64 array or
    None).  Exactly what columnar._encode_keys gives for the same strings
    passed as a list: UTF-8 byte order is code-point order, and the table is
    sorted as str in any case.

    hash -> dpg_keydict_insert_slots into a table sized by `max_distinct`
    (else by n, as distributed._pid_capacity) -> one representative record per
    slot -> byte compare of every record with its representative -> ONE host
    synchronisation reading the distinct, invalid-offset, lost and mismatch
    counts together -> the D representative strings to the host, decoded and
    sorted -> every occupied slot gets its rank -> dpg_keydict_gather_ids.
    Memory: 8 B key and 4 B slot per record, 12 B per table slot (the 8 B key
    slot and the 4 B representative, whose array then carries the slot's id).

    ValueError, after the one synchronisation and before anything else runs:
    invalid offsets, a table that overflowed, or records whose bytes differ
    from their slot's representative (a 64-bit hash collision)."""
    from . import distributed
    offsets, data = column.device_columns(device)
    n = len(column)
    if n >= 1 << 31:
        raise ValueError("a string column holds 2^31 or more records; a device takes fewer")
    capacity = distributed._pid_capacity(n, max_distinct)
    with torch.cuda.device(device):
        sptr = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        keys, n_invalid = device_keys(offsets, data, column.hash_seed, ctx, sptr)
        slots = torch.full((capacity,), _I64_MIN, dtype=torch.int64, device=device)
        info = torch.zeros(2, dtype=torch.int64, device=device)
        rec_slots = torch.empty(n, dtype=torch.int32, device=device)  # uint32 bit patterns
        ctx.keydict_insert_slots(keys.data_ptr(), n, slots.data_ptr(), capacity,
                                 rec_slots.data_ptr(), info.data_ptr(), sptr)
        del keys, slots
        rep = torch.full((capacity,), -1, dtype=torch.int32, device=device)  # 0xFFFFFFFF
        ctx.keydict_representatives(rec_slots.data_ptr(), n, capacity, rep.data_ptr(), sptr)
        n_mismatch = torch.zeros(1, dtype=torch.int64, device=device)
        ctx.string_verify(offsets.data_ptr(), data.data_ptr(), data.numel(), n,
                          rec_slots.data_ptr(), rep.data_ptr(), n_mismatch.data_ptr(), sptr)
        has_rep = rep != -1
        # the one host synchronisation
        D, invalid, _, lost, mismatch = torch.cat(
            [torch.count_nonzero(has_rep).reshape(1), n_invalid, info, n_mismatch]).tolist()
        if invalid:
            raise ValueError(f"{invalid} records of the partition key StringColumn have offsets "
                             f"outside 0 <= offsets[i] <= offsets[i + 1] <= len(data)")
        if lost:
            raise ValueError(
                f"string partition keys: the key table sized by max_distinct_partition_keys="
                f"{max_distinct} overflowed ({lost} records found no slot); raise "
                f"max_distinct_partition_keys to at least the number of distinct partition keys")
        if mismatch:
            raise ValueError(f"{mismatch} records share a 64-bit hash with a different string; "
                             f"pass another hash_seed")
        occupied = torch.nonzero_static(has_rep, size=D).view(-1)
        distinct = _gather_strings(offsets, data, rep[occupied].to(torch.int64), column.encoding)
        table = sorted(set(distinct).union(public or ()))
        index = {s: i for i, s in enumerate(table)}
        # the representatives have done their work: their array carries the ids
        slot_ids = rep
        slot_ids[occupied] = torch.tensor([index[s] for s in distinct], dtype=torch.int32,
                                          device=device)
        ids = torch.empty(n, dtype=torch.int64, device=device)
        n_missing = torch.zeros(1, dtype=torch.int64, device=device)
        ctx.keydict_gather_ids(rec_slots.data_ptr(), n, slot_ids.data_ptr(), capacity,
                               ids.data_ptr(), n_missing.data_ptr(), sptr)
    public_ids = (None if public is None
                  else np.asarray([index[s] for s in public], dtype=np.int64))
    return ids, table, public_ids


def encode_global_partition_keys(column: StringColumn, public: Optional[List[str]], device, ctx,
                                 max_distinct: Optional[int] = None, group=None):
    """ColumnarData(global_string_keys=True): the ids of a string partition
    column from the global string dictionary, on one rank (`group` None) or
    several -- distributed.build_string_dictionary, which see; returns its
    StringDictionary (ids of the records and of `public`, P, and this rank's
    slice of the string table, on the device).  Unlike `encode_partition_keys`
    the ids are the ascending rank of the HASHES (i * R + owner), no string is
    decoded or sorted here, and none reaches the host before a partition is
    kept."""
    from . import distributed
    with torch.cuda.device(device):
        return distributed.build_string_dictionary(column, public, group, ctx, device,
                                                   max_distinct=max_distinct)
