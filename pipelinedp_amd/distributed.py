"""Multi-GPU exchange of the per-partition partials (one process per GPU).

Contribution bounding is shard-local: it is correct only if each privacy id
lives on exactly one rank, the rank `shard_of(pid, R)`.  Three ways to get
there (`ColumnarData(sharding=...)`):

* "trusted" (default) -- the caller sharded the records that way; nothing is
  checked and no collective is added.  Records split any other way (by file,
  by time, round-robin) release up to R x max_partitions_contributed
  partitions per privacy id, unreported.
* "verify" -- the same claim, checked: one kernel counts the records a rank
  holds but does not own (dpg_check_shard), ONE all_reduce sums the counts,
  and every rank raises ValueError when the sum is nonzero.
* "shuffle" -- any split: `shuffle_records` orders each rank's records by
  owner on the device (dpg_shard_records: a stable multi-way split) and ONE
  all_to_all per column delivers them, as the reference's framework shuffle
  groups each privacy id's records before sampling
  (contribution_bounders.py:86-92).  Bounding then runs on the received
  records with record id offset 0.

What a shuffled release guarantees.  Pair sampling is keyed by (seed, pid, pk)
only and each privacy id's pairs are all on one rank, so `rows`, the selected
partition set and -- in the cross-and-per-partition and cross-partition modes,
where a pair counts min(len, max_contributions_per_partition) -- `count` equal
the one-process release of the whole dataset under the same seed and nonce.
The record sampler is keyed by record id, which after a shuffle is the
record's position in the received buffer (source rank order, input order
within a source: deterministic): which records of an over-full pair are kept
is still uniform and the release is correctly bounded, but `sum` in every
mode and `count` under `max_contributions` may differ from the one-process
release; they equal the release of each rank's received records.

With the records in place the only further exchange is the merge of the
per-partition partials -- and, for a plan with percentiles or VECTOR_SUM,
of the kept items behind it: `exchange_owner_keys` sends partition-keyed
items (sorted tree keys; the occupied partitions' summed rows) to the
partitions' owners, ordered by one stable split on the device
(dpg_owner_split_keys) whose R counts are read back: one more host
synchronisation per release.

The utility analysis moves whole pre-aggregate entries the same way:
`exchange_owner_pairs` splits a rank's pk-sorted (privacy id, partition) pairs
by owner (dpg_owner_split_pairs), sends them in ONE all_to_all and merges the
R sorted runs it receives into the owned slice's pre-aggregate
(dpg_merge_pair_runs).  The per-partition utility combiners are not sums over
ranks -- the selection probability is a convolution over a partition's pairs
-- so the pairs, not partials, have to meet.

The dataset histograms move neither records nor pairs: their bins are sums
over ranks once the per-partition totals (`exchange_partials` of rows and
count) and the range of the pair sums (`hist_header`) are global;
`merge_histograms` then adds and maxes the bins in three all_reduces
(DESIGN.md section 14).

Ownership is by partition key: rank r owns partitions r, r + R, r + 2R, ...
(R ranks; `pk mod R`, the identity hash of the dense ids), at local index
pk // R.  Interleaving spreads hot low ids -- an unpermuted Zipf key space
puts most of its occupied partitions at the bottom -- over every rank, so the
sparse exchange's receive volume and every rank's selection work stay
balanced whatever the key order.  The owner runs selection + noise for its
partitions and the kept results are all-gathered (SURVEY.md 8(e);
DESIGN.md section 5).  Two exchanges reach the owner:

* dense -- ONE `reduce_scatter` (sum) of all accumulator arrays packed
  together: 8 B x (A x S + 1) per destination, S = ceil(P / R) (A =
  accumulator arrays; P = 1e6, COUNT+SUM+PID: 24 MB per rank), whatever
  the occupancy;
* sparse -- ONE `all_to_all` with equal splits: every destination gets a
  fixed block of `cap` rows (pk, partial_1..A) (padding rows pk = -1), cap =
  min(S, an upper bound on the partitions one rank can occupy), so no count
  exchange and no host round trip of split sizes is needed.

Neither exchange synchronises the host: the choice between them is made
from host-known sizes only (`choose_exchange`: P, A, R and the occupancy
bound min(P, records, privacy ids x l0), maximised over ranks in the one
collective that already carries the release nonce, `release_header`), and
the split sizes are static.  Every block also carries its sender's
internal-error flag (a bounding whose table overflowed); the owner latches
the sum (`dpg_import_error`), so an error on any rank fails every rank's
`dpg_compact_kept` instead of releasing partials of a mis-bounded shard.

The integer accumulators travel as float64, exact below 2^53 (a rank holds
< 2^32 records).  With gloo (CPU tests, and several ranks sharing one GPU)
the collectives are staged through host memory and the reduce-scatter is an
all_reduce + slice.

Partition keys that are not dense ids (ColumnarData(sparse_partition_keys=
True): any int64 but INT64_MIN) get them first: `build_key_dictionary` reduces
each rank's records to their distinct keys in a write-once hash table on the
device, sends those to the ranks `key_owner` names, numbers them there so that
id % R is that owner, and maps every record through the table (DESIGN.md
section 16).  The kept results then carry the caller's keys
(`all_gather_results(exact_ids=True)`).

Privacy ids that span more than 2^32 values (ColumnarData(wide_privacy_ids=
True): any int64 but INT64_MIN) are owned by `shard_of_wide`, a hash of all 64
bits, in all three sharding modes, and get dense ids rank by rank once the
records are in place: `encode_privacy_ids` numbers each rank's distinct ids in
the same kind of hash table, probed once per record, and adds one all_reduce
that makes every rank raise the same error.

A StringColumn of privacy ids (string_columns.py) is
hashed to such wide ids when the input is encoded, so all of the above holds
for it: the owner of a string is `shard_of_wide(string_key_hash(column), R)`.
Records with invalid offsets are counted on the device and travel in
`encode_privacy_ids`' all_reduce, so every rank raises for them together.  A
StringColumn of partition keys is one-process only unless
ColumnarData(global_string_keys=True) asks for `build_string_dictionary`: ids
from the hashes through `build_key_dictionary`, one representative string per
hash sent to the hash's owner, which verifies the strings arriving under one
hash and keeps its slice of the string table.

Every random draw is keyed by (stream seed, pid, pk) or (stream seed, pk)
with global partition ids -- never by rank -- and the release nonce comes
from rank 0, so the selected-partition set is identical for any world size
(SURVEY.md 8(e)).
"""
import ctypes
import dataclasses
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import string_columns

_PACK_ORDER = ("rows", "count", "sum", "nsum", "nsq")
_PACK_DTYPE = {"rows": torch.int64, "count": torch.int64, "sum": torch.float64,
               "nsum": torch.float64, "nsq": torch.float64}
_I64_MIN = -(1 << 63)


def shard_of(pid: torch.Tensor, world_size: int) -> torch.Tensor:
    """Rank owning each privacy id (multiplicative hash, independent of the
    bits the kernels bucket by)."""
    h = (pid.to(torch.int64) * 0x9E3779B1) & 0xFFFFFFFF
    return ((h * world_size) >> 32).to(torch.int64)


def shard_of_wide(pid, world_size: int) -> torch.Tensor:
    """Rank owning each wide privacy id (ColumnarData(wide_privacy_ids=True)):
    `key_owner`, ((fmix64(pid) >> 32) * R) >> 32 -- a hash of all 64 bits, where
    `shard_of` reads the low 32 only and sends ids that differ above them
    (user << 32) to one rank.  Device form: dpg_shard_records_wide,
    dpg_check_shard_wide."""
    return key_owner(pid, world_size)


def string_key_hash(column, ctx=None) -> torch.Tensor:
    """The 64-bit keys (int64 bit patterns) of a StringColumn's records: what
    a string privacy id becomes, so a caller can pre-shard for "trusted" with
    shard_of_wide(string_key_hash(column), R).  A column whose tensors are on
    the device is hashed there (dpg_string_hash, with the library context
    `ctx` or a temporary one) and the keys stay there; any other column is
    hashed by the numpy restatement (string_columns.host_keys).  Records with
    invalid offsets get the key 0; the encoder raises for them."""
    if column.is_on_device():
        dev = column.offsets.device
        if ctx is None:
            from . import _native
            ctx = _native.Context(dev.index if dev.index is not None
                                  else torch.cuda.current_device(), 0)
        keys, _ = string_columns.device_keys(*column.device_columns(dev), column.hash_seed, ctx)
        return keys
    keys, _ = string_columns.host_keys(*column.host_columns(), column.hash_seed)
    return torch.from_numpy(keys)


def owned(P: int, world_size: int, rank: int) -> Tuple[int, int, int]:
    """(lo, stride, n): this rank owns partitions lo + i * stride, i < n."""
    n = (P - rank + world_size - 1) // world_size if rank < P else 0
    return rank, world_size, n


def owner_of(pk: torch.Tensor, world_size: int) -> torch.Tensor:
    return pk.to(torch.int64) % world_size


def _is_nccl(group) -> bool:
    return dist.get_backend(group) == "nccl"


def _coll_device(group, device):
    return device if _is_nccl(group) else torch.device("cpu")


def broadcast_u64(x: int, group, device) -> int:
    """Rank 0's 64-bit value on every rank."""
    return release_header(x, 0, group, device)[0]


def release_header(nonce: int, nnz_bound: int, group, device) -> Tuple[int, int]:
    """ONE all_reduce (max) before a release: rank 0's nonce (the others
    contribute INT64_MIN) and the largest occupancy bound over ranks, so
    every rank draws the same streams and takes the same exchange."""
    signed = nonce - (1 << 64) if nonce >= (1 << 63) else nonce
    root = dist.get_global_rank(group, 0) if group is not None else 0
    mine = signed if dist.get_rank() == root else _I64_MIN
    t = torch.tensor([mine, int(nnz_bound)], dtype=torch.int64,
                     device=_coll_device(group, device))
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    got = t.tolist()
    return got[0] & ((1 << 64) - 1), got[1]


def sum_over_ranks(x: torch.Tensor, group) -> int:
    """ONE all_reduce (sum) of a one-element int64 tensor; the total on every
    rank (sharding='verify': the mis-sharded records of all ranks)."""
    t = x.to(_coll_device(group, x.device)).reshape(1).clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return int(t.item())


def _exchange_column(send: torch.Tensor, in_splits, out_splits, group) -> torch.Tensor:
    """One all_to_all_single of a destination-major column with uneven
    splits (on gloo staged through host memory)."""
    dev = send.device
    if _is_nccl(group):
        recv = torch.empty(sum(out_splits), dtype=send.dtype, device=dev)
        dist.all_to_all_single(recv, send, out_splits, in_splits, group=group)
        return recv
    recv = torch.empty(sum(out_splits), dtype=send.dtype, device="cpu")
    dist.all_to_all_single(recv, send.cpu(), out_splits, in_splits, group=group)
    return recv.to(dev)


def _split_sizes(counts: torch.Tensor, group, dev, what: str, items: str):
    """ONE all_gather of this rank's R send counts (host int64[R]): every rank
    then holds the R x R matrix [source, destination], so its own send and
    receive splits; a receive total of 2^31 or more on any rank raises the
    same ValueError on every rank."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    cdev = _coll_device(group, dev)
    rows = [torch.empty(world, dtype=torch.int64, device=cdev) for _ in range(world)]
    dist.all_gather(rows, counts.to(cdev), group=group)
    matrix = torch.stack(rows).cpu()  # [source, destination]
    worst = int(matrix.sum(0).max().item())
    if worst >= 1 << 31:
        raise ValueError(f"{what}: one rank would receive {worst} {items}; a rank "
                         f"holds fewer than 2^31")
    return matrix[rank].tolist(), matrix[:, rank].tolist()


def shuffle_records(pid: torch.Tensor, pk: torch.Tensor, value: Optional[torch.Tensor], group,
                    ctx=None, stream=None, wide: bool = False):
    """Delivers every record to the rank `shard_of(pid, R)` -- wide=True (wide
    privacy ids): `shard_of_wide(pid, R)`, dpg_shard_records_wide; returns this
    rank's (pid, pk, value) in source-rank order, input order within a source
    (value None stays None: every rank must pass None or none of them; a
    [n, D] value -- VECTOR_SUM rows, D the same on every rank -- travels row
    by row).

    Device tensors with the library context `ctx`: the send order is ONE
    stable split on the device (dpg_shard_records, stream-ordered on `stream`,
    torch's current stream); reading its R counts back is the shuffle's one
    host synchronisation -- the receive sizes must be known.  Host tensors
    (the gloo CPU tests, no context): the same layout from a stable argsort
    of shard_of and a bincount.

    Every rank runs the same collectives whatever its local n: one all_gather
    of the R counts (every rank then holds the R x R matrix, so its own send
    and receive splits, and sees a receive total of 2^31 or more on any rank:
    all ranks then raise the same ValueError), and one all_to_all_single per
    column.  The send buffers are freed column by column."""
    world = dist.get_world_size(group)
    dev = pid.device
    n = pid.numel()
    pid = pid.to(torch.int64).contiguous()
    pk = pk.to(torch.int64).contiguous()
    if value is not None:
        value = value.to(torch.float64).contiguous()
    rows = value is not None and value.dim() == 2  # VECTOR_SUM: [n, D]
    if ctx is not None and dev.type == "cuda":
        s_pid, s_pk = torch.empty_like(pid), torch.empty_like(pk)
        # the split moves one 8-byte value column: rows of vectors follow the
        # record positions it moved in their place (exact in float64)
        col = torch.arange(n, dtype=torch.float64, device=dev) if rows else value
        s_val = torch.empty_like(col) if col is not None else None
        counts = torch.empty(world, dtype=torch.int64, device=dev)
        split = ctx.shard_records_wide if wide else ctx.shard_records
        split(pid.data_ptr(), pk.data_ptr(), col.data_ptr() if col is not None else None, n,
              world, s_pid.data_ptr(), s_pk.data_ptr(),
              s_val.data_ptr() if s_val is not None else None, counts.data_ptr(), stream)
        if rows:
            s_val = value.index_select(0, s_val.to(torch.int64))
        del col
        counts = counts.cpu()  # the one host synchronisation
    else:
        dest = shard_of_wide(pid, world) if wide else shard_of(pid, world)
        order = torch.argsort(dest, stable=True)
        counts = torch.bincount(dest, minlength=world).cpu()
        s_pid, s_pk = pid[order], pk[order]
        s_val = value[order] if value is not None else None
    del pid, pk, value
    in_splits, out_splits = _split_sizes(counts, group, dev, "record shuffle", "records")
    r_pid = _exchange_column(s_pid, in_splits, out_splits, group)
    del s_pid
    r_pk = _exchange_column(s_pk, in_splits, out_splits, group)
    del s_pk
    r_val = None
    if s_val is not None and rows:
        D = s_val.shape[1]
        r_val = _exchange_column(s_val.view(-1), [c * D for c in in_splits],
                                 [c * D for c in out_splits], group).view(-1, D)
    elif s_val is not None:
        r_val = _exchange_column(s_val, in_splits, out_splits, group)
    del s_val
    return r_pid, r_pk, r_val


def exchange_owner_keys(keys: torch.Tensor, n_keys, low_bits: int, group, ctx=None, stream=None,
                        payload: Optional[torch.Tensor] = None):
    """Delivers partition-keyed items to the rank that owns their partition.

    keys: int64 tensor holding the 64-bit keys pk << low_bits | low; the first
    n_keys of them count (a one-element int64 tensor -- on the keys' device,
    so the count never reaches the host before the split -- an int, or None:
    all).  Key k goes to rank `owner_of(pk)` = pk % R and arrives re-based to
    the owner's local partition id: (pk // R) << low_bits | low.  payload: a
    [n, D] float64 tensor (D the same on every rank; every rank passes one or
    none does) whose row i travels with key i.

    Returns (keys, payload or None, total): what this rank received, in
    source-rank order, input order within a source, and its length.

    Device tensors with the library context `ctx`: the send order is ONE
    stable split on the device (dpg_owner_split_keys, stream-ordered on
    `stream`, torch's current stream); reading its R counts back is the
    exchange's one host synchronisation.  Host tensors (the gloo CPU tests,
    no context): the same layout from a stable argsort of pk % R.

    Every rank runs the same collectives whatever its local count, zero
    included: one all_gather of the R counts (`_split_sizes`: a receive total
    of 2^31 or more on any rank raises the same ValueError everywhere), one
    all_to_all_single of the keys and, with a payload, a second one of its
    rows gathered destination-major."""
    world = dist.get_world_size(group)
    dev = keys.device
    keys = keys.to(torch.int64).contiguous().view(-1)
    n_max = keys.numel()
    if payload is not None:
        payload = payload.to(torch.float64).contiguous()
    if ctx is not None and dev.type == "cuda":
        if not isinstance(n_keys, torch.Tensor):
            n_keys = torch.tensor([n_max if n_keys is None else int(n_keys)], dtype=torch.int64,
                                  device=dev)
        s_keys = torch.empty_like(keys)
        src = torch.empty(n_max, dtype=torch.int32, device=dev) if payload is not None else None
        counts = torch.empty(world, dtype=torch.int64, device=dev)
        ctx.owner_split_keys(keys.data_ptr(), n_keys.data_ptr(), n_max, int(low_bits), world,
                             s_keys.data_ptr(), src.data_ptr() if src is not None else None,
                             counts.data_ptr(), stream)
        counts = counts.cpu()  # the one host synchronisation
        sent = int(counts.sum().item())
        s_keys = s_keys[:sent]
        if src is not None:
            src = src[:sent].to(torch.int64)  # positions < 2^31
    else:
        n = n_max if n_keys is None else int(n_keys)
        keys = keys[:n]
        # a logical shift: a key with bit 63 set is a negative int64
        pk = (keys >> low_bits) & ((1 << (64 - low_bits)) - 1) if low_bits else keys
        dest = pk % world
        src = torch.argsort(dest, stable=True)
        counts = torch.bincount(dest, minlength=world).cpu()
        s_keys = (((pk // world) << low_bits) | (keys & ((1 << low_bits) - 1)))[src]
    del keys
    in_splits, out_splits = _split_sizes(counts, group, dev, "owner exchange", "keys")
    r_keys = _exchange_column(s_keys, in_splits, out_splits, group)
    del s_keys
    r_pay = None
    if payload is not None:
        D = payload.shape[1]
        rows = payload.index_select(0, src).view(-1)
        r_pay = _exchange_column(rows, [c * D for c in in_splits], [c * D for c in out_splits],
                                 group).view(-1, D)
    return r_keys, r_pay, sum(out_splits)


DENSE_IDS_ERROR = ("multi-GPU aggregation needs globally dense integer partition ids: "
                   "pass ColumnarData(..., n_partitions=P) with pk in [0, P) on every rank")


def _as_i64(c: int) -> int:
    return c - (1 << 64) if c >= 1 << 63 else c


def _lsr(x: torch.Tensor, bits: int) -> torch.Tensor:
    """Logical shift right of int64 bit patterns."""
    return (x >> bits) & ((1 << (64 - bits)) - 1)


def key_hash(keys) -> torch.Tensor:
    """fmix64 (murmur3's 64-bit finaliser) of int64 keys, as int64 bit
    patterns: the hash of the device key dictionary (csrc/dpg_keydict.h), bit
    for bit.  A key's home slot in a table of `capacity` slots is
    key_hash(key) & (capacity - 1)."""
    k = torch.as_tensor(keys).to(torch.int64)
    k = k ^ _lsr(k, 33)
    k = k * _as_i64(0xff51afd7ed558ccd)  # int64 products wrap: arithmetic mod 2^64
    k = k ^ _lsr(k, 33)
    k = k * _as_i64(0xc4ceb9fe1a85ec53)
    return k ^ _lsr(k, 33)


def key_owner(keys, world_size: int) -> torch.Tensor:
    """Rank owning each sparse partition key: ((h >> 32) * R) >> 32 with h =
    key_hash(key) -- the hash's high half, independent of the slot bits."""
    return (_lsr(key_hash(keys), 32) * int(world_size)) >> 32


@dataclasses.dataclass
class KeyDictionary:
    """What build_key_dictionary returns (see there)."""
    ids: torch.Tensor                    # int64: the global dense id of every record
    public_ids: Optional[torch.Tensor]   # the same for the public keys, or None
    n_partitions: int                    # P, the same on every rank
    owned_keys: torch.Tensor             # this rank's owned keys, int64, ascending
    keys: torch.Tensor                   # this rank's distinct keys, ascending
    key_ids: torch.Tensor                # their global ids


def build_key_dictionary(pk: torch.Tensor, public_keys: Optional[torch.Tensor], group, ctx=None,
                         stream=None, max_distinct: Optional[int] = None) -> KeyDictionary:
    """Global dense ids for sparse int64 partition keys, the same on every rank.

    pk: this rank's record keys (any int64 but INT64_MIN, which the device
    table reserves); public_keys: the public partition keys, the same on every
    rank, or None.  group: the process group; None = one process (R = 1, no
    collective).

    1. Local distinct keys.  Device tensors with the library context `ctx`:
       one probe per record into a write-once hash table of capacity = the
       power of two >= 2 * min(records + public keys, max_distinct), at least
       64 (dpg_keydict_insert; 12 bytes per slot plus 8 for the compaction, so
       max_distinct is what keeps the table small when the records outnumber
       their keys), compacted (dpg_keydict_keys; reading the count back is
       host synchronisation 1) and sorted ascending as signed values
       (dpg_sort_pairs_u64 on key ^ 2^63).  Host tensors (the gloo CPU tests,
       no context): torch.unique.
    2. To owners: the sorted distinct keys are split by key_owner (torch ops:
       the column is the distinct keys, not the records; reading the R counts
       is host synchronisation 2), `_split_sizes` and one all_to_all_single.
    3. At the owner: what arrived is sorted and adjacent duplicates dropped --
       `owned_keys`; the key at position i gets the global id i * R + rank, so
       id % R is its owner (owner_of) and id // R indexes owned_keys.  The ids
       go back in arrival order with one all_to_all_single.
    4. ONE all_reduce (sum) carries every rank's len(owned_keys) in a slot of
       its own, the records holding the reserved key and the records that
       found no slot.  P = R * max(len(owned_keys)) (at least R).  No rank
       raises before this collective; after it all raise the same ValueError:
       a reserved key, a table that overflowed (only with max_distinct; the
       message names it), or P >= 2^32 - 1.
    5. Map: dpg_keydict_assign stores the ids beside the rank's distinct keys
       and dpg_keydict_lookup reads every record's and every public key's
       (host tensors: searchsorted).  A key without an id is an internal error
       (RuntimeError; its count is read back behind the lookups).

    The ids between an owner's own key count and P / R are holes: no key has
    them.  With R = 1 the ids are the ascending rank of each key, as
    torch.unique(return_inverse=True) numbers them.  They depend only on the
    union of the key sets and on R.  Every rank runs every collective (four:
    the all_gather of `_split_sizes`, two all_to_all_single, one all_reduce),
    a rank without records included."""
    world = 1 if group is None else dist.get_world_size(group)
    rank = 0 if group is None else dist.get_rank(group)
    pk = pk.to(torch.int64).contiguous().view(-1)
    dev = pk.device
    if public_keys is not None:
        public_keys = public_keys.to(torch.int64).to(dev).contiguous().view(-1)
    n, m = pk.numel(), public_keys.numel() if public_keys is not None else 0
    on_device = ctx is not None and dev.type == "cuda"
    # ---- 1. local distinct keys, ascending
    if on_device:
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        bound = n + m if max_distinct is None else min(n + m, max(0, int(max_distinct)))
        capacity = max(64, 1 << max(2 * bound - 1, 0).bit_length())
        slots = torch.full((capacity,), _I64_MIN, dtype=torch.int64, device=dev)
        info = torch.zeros(2, dtype=torch.int64, device=dev)
        ctx.keydict_insert(pk.data_ptr(), n, slots.data_ptr(), capacity, info.data_ptr(), stream)
        if m:
            ctx.keydict_insert(public_keys.data_ptr(), m, slots.data_ptr(), capacity,
                               info.data_ptr(), stream)
        found = torch.empty(capacity, dtype=torch.int64, device=dev)
        n_found = torch.empty(1, dtype=torch.int64, device=dev)
        ctx.keydict_keys(slots.data_ptr(), capacity, found.data_ptr(), n_found.data_ptr(), stream)
        cnt = int(n_found.item())  # host synchronisation 1
        biased = found[:cnt] ^ _I64_MIN  # unsigned order of key ^ 2^63 = signed order of key
        distinct = torch.empty_like(biased)
        ctx.sort_pairs_u64(biased.data_ptr(), None, cnt, 0, 64, distinct.data_ptr(), None, stream)
        distinct ^= _I64_MIN
        del found, biased
        errs = info
    else:
        both = pk if not m else torch.cat([pk, public_keys])
        distinct = torch.unique(both)
        n_reserved = int((both == _I64_MIN).sum().item())
        distinct = distinct[distinct != _I64_MIN]
        cnt = int(distinct.numel())
        lost = 0
        if max_distinct is not None:  # the device table's capacity, mirrored
            capacity = max(64, 1 << max(2 * min(n + m, max(0, int(max_distinct))) - 1,
                                        0).bit_length())
            lost = max(0, cnt - capacity)
        errs = torch.tensor([n_reserved, lost], dtype=torch.int64)
    # ---- 2. to owners (ascending within a destination: the split is stable)
    if world > 1:
        dest = key_owner(distinct, world)
        order = torch.argsort(dest, stable=True)
        counts = torch.bincount(dest, minlength=world).cpu()  # host synchronisation 2
        in_splits, out_splits = _split_sizes(counts, group, dev, "key dictionary", "keys")
        arrived = _exchange_column(distinct[order], in_splits, out_splits, group)
        # ---- 3. at the owner
        total = int(arrived.numel())
        if on_device:
            biased = arrived ^ _I64_MIN
            srt = torch.empty_like(biased)
            ctx.sort_pairs_u64(biased.data_ptr(), None, total, 0, 64, srt.data_ptr(), None, stream)
            owned_keys = torch.unique_consecutive(srt ^ _I64_MIN)
        else:
            owned_keys = torch.unique(arrived)
        back = torch.searchsorted(owned_keys, arrived) * world + rank
        got = _exchange_column(back, out_splits, in_splits, group)
        key_ids = torch.empty_like(got)
        key_ids[order] = got
    else:
        owned_keys = distinct
        key_ids = torch.arange(cnt, dtype=torch.int64, device=dev)
    # ---- 4. global size and errors
    n_owned = int(owned_keys.numel())
    if world > 1:
        cdev = _coll_device(group, dev)
        t = torch.zeros(world + 2, dtype=torch.int64, device=cdev)
        t[rank] = n_owned
        t[world:] = errs.to(cdev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        t = t.tolist()
        n_owned, n_reserved, n_lost = max(t[:world]), t[world], t[world + 1]
    else:
        n_reserved, n_lost = errs.tolist()
    P = world * max(1, n_owned)
    if n_reserved:
        raise ValueError(
            f"sparse partition keys: {n_reserved} records or public partitions hold the key "
            f"INT64_MIN (-2^63), which the key dictionary reserves")
    if n_lost:
        raise ValueError(
            f"sparse partition keys: the key dictionary sized by max_distinct={max_distinct} "
            f"overflowed ({n_lost} records found no slot on their rank); raise max_distinct to at "
            f"least the number of distinct partition keys of one rank")
    if P >= (1 << 32) - 1:
        raise ValueError(f"sparse partition keys: {P} partition ids; the kernels take fewer "
                         f"than 2^32 - 1")
    # ---- 5. map
    if on_device:
        slot_ids = torch.empty(capacity, dtype=torch.int32, device=dev)
        n_missing = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.keydict_assign(distinct.data_ptr(), key_ids.data_ptr(), cnt, slots.data_ptr(),
                           slot_ids.data_ptr(), capacity, n_missing.data_ptr(), stream)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        ctx.keydict_lookup(pk.data_ptr(), n, slots.data_ptr(), slot_ids.data_ptr(), capacity,
                           ids.data_ptr(), n_missing.data_ptr(), stream)
        public_ids = None
        if public_keys is not None:
            public_ids = torch.empty(m, dtype=torch.int64, device=dev)
            ctx.keydict_lookup(public_keys.data_ptr(), m, slots.data_ptr(), slot_ids.data_ptr(),
                               capacity, public_ids.data_ptr(), n_missing.data_ptr(), stream)
        missing = int(n_missing.item())
    else:
        def lookup(x):
            pos = torch.searchsorted(distinct, x).clamp_(max=max(cnt - 1, 0))
            hit = distinct[pos] == x if cnt else torch.zeros_like(x, dtype=torch.bool)
            return (key_ids[pos] if cnt else torch.full_like(x, -1)), int((~hit).sum().item())
        ids, missing = lookup(pk)
        public_ids = None
        if public_keys is not None:
            public_ids, miss_pub = lookup(public_keys)
            missing += miss_pub
    if missing:
        raise RuntimeError(f"key dictionary: {missing} keys have no id (internal error)")
    return KeyDictionary(ids=ids, public_ids=public_ids, n_partitions=P, owned_keys=owned_keys,
                         keys=distinct, key_ids=key_ids)


@dataclasses.dataclass
class StringDictionary:
    """What build_string_dictionary returns (see there)."""
    ids: torch.Tensor                    # int64: the global dense id of every record
    public_ids: Optional[torch.Tensor]   # the same for the public strings, or None
    n_partitions: int                    # P, the same on every rank
    owned_keys: torch.Tensor             # this rank's owned hashes, int64, ascending
    owned_offsets: torch.Tensor          # int64[n_owned + 1]: the owned string table,
    owned_data: torch.Tensor             # uint8, in owned_keys order
    encoding: str = "utf-8"
    ctx: Any = None                      # the library context the table is packed with

    def packed(self, local_ids: torch.Tensor):
        """(offsets int64[k + 1], bytes uint8) of the owned strings at the
        given local ids (global id // R), packed on the table's device
        (string_columns.pack_strings)."""
        out_offsets, out_data, bad = string_columns.pack_strings(
            self.owned_offsets, self.owned_data,
            local_ids.to(torch.int64).to(self.owned_offsets.device), self.ctx)
        if int(bad.item()):
            raise RuntimeError(f"string dictionary: {int(bad.item())} kept ids have no owned "
                               f"string (internal error)")
        return out_offsets, out_data

    def strings(self, local_ids: torch.Tensor) -> list:
        """The owned strings at the given local ids, decoded on the host."""
        return string_columns.decode_packed(*self.packed(local_ids), self.encoding)


STRING_OFFSETS_ERROR = ("{} records of the partition key StringColumn have offsets "
                        "outside 0 <= offsets[i] <= offsets[i + 1] <= len(data)")
STRING_OVERFLOW_ERROR = (
    "string partition keys: the key table sized by max_distinct_partition_keys="
    "{} overflowed ({} records found no slot); raise "
    "max_distinct_partition_keys to at least the number of distinct partition keys")
STRING_COLLISION_ERROR = ("{} records or strings share a 64-bit hash with a different string; "
                          "pass another hash_seed")


def _local_string_keys(column, dev, ctx, sptr, max_distinct):
    """Step 1 of build_string_dictionary on this rank: returns (offsets, data,
    hashes int64[D] of the distinct strings, their representative records
    int64[D], finish, [invalid offsets, lost, local mismatches]); finish(ids
    int64[D]) gives every record the id of its string."""
    n = len(column)
    if n >= 1 << 31:
        raise ValueError("a string column holds 2^31 or more records; a device takes fewer")
    capacity = _pid_capacity(n, max_distinct)
    if ctx is not None and dev.type == "cuda":
        offsets, data = column.device_columns(dev)
        keys, n_invalid = string_columns.device_keys(offsets, data, column.hash_seed, ctx, sptr)
        slots = torch.full((capacity,), _I64_MIN, dtype=torch.int64, device=dev)
        info = torch.zeros(2, dtype=torch.int64, device=dev)
        rec_slots = torch.empty(n, dtype=torch.int32, device=dev)  # uint32 bit patterns
        ctx.keydict_insert_slots(keys.data_ptr(), n, slots.data_ptr(), capacity,
                                 rec_slots.data_ptr(), info.data_ptr(), sptr)
        del slots
        rep = torch.full((capacity,), -1, dtype=torch.int32, device=dev)  # 0xFFFFFFFF
        ctx.keydict_representatives(rec_slots.data_ptr(), n, capacity, rep.data_ptr(), sptr)
        n_mismatch = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.string_verify(offsets.data_ptr(), data.data_ptr(), data.numel(), n,
                          rec_slots.data_ptr(), rep.data_ptr(), n_mismatch.data_ptr(), sptr)
        has_rep = rep != -1
        # the one host synchronisation of the local step
        D, invalid, _, lost, mismatch = torch.cat(
            [torch.count_nonzero(has_rep).reshape(1), n_invalid, info, n_mismatch]).tolist()
        occupied = torch.nonzero_static(has_rep, size=D).view(-1)
        rep_rec = rep[occupied].to(torch.int64)
        hashes = keys[rep_rec]
        del keys, has_rep

        def finish(ids: torch.Tensor) -> torch.Tensor:
            # the representatives have done their work: their array carries the ids
            rep[occupied] = ids.to(torch.int32)
            out = torch.empty(n, dtype=torch.int64, device=dev)
            n_missing = torch.zeros(1, dtype=torch.int64, device=dev)
            ctx.keydict_gather_ids(rec_slots.data_ptr(), n, rep.data_ptr(), capacity,
                                   out.data_ptr(), n_missing.data_ptr(), sptr)
            return out
        return offsets, data, hashes, rep_rec, finish, [invalid, lost, mismatch]
    # host tensors: the same outcome from numpy (first-seen record = representative)
    h_off, h_data = column.host_columns()
    keys, invalid = string_columns.host_keys(h_off, h_data, column.hash_seed)
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    # the device table's capacity, mirrored: the keys past it find no slot
    fits = np.ones(uniq.size, dtype=bool)
    if uniq.size > capacity:
        fits[np.argsort(first, kind="stable")[capacity:]] = False
    lost = int((~fits[inv]).sum())
    start, length, ok = string_columns._np_ranges(h_off, h_data.size, n, np.arange(n))
    buf = h_data.tobytes()
    raw = [buf[a:a + ln] if v else None for a, ln, v in zip(start.tolist(), length.tolist(),
                                                           ok.tolist())]
    mismatch = sum(1 for i, u in enumerate(inv.tolist())
                   if fits[u] and (raw[i] is None or raw[i] != raw[first[u]]))
    new_index = np.cumsum(fits) - 1  # position of a key among the kept ones
    rep_rec = torch.from_numpy(first[fits].astype(np.int64))
    hashes = torch.from_numpy(uniq[fits].astype(np.int64))

    def finish(ids: torch.Tensor) -> torch.Tensor:
        out = np.full(n, -1, dtype=np.int64)
        kept = fits[inv]
        out[kept] = ids.numpy()[new_index[inv[kept]]]
        return torch.from_numpy(out)
    return (torch.from_numpy(h_off), torch.from_numpy(h_data), hashes, rep_rec, finish,
            [int(invalid), lost, mismatch])


def build_string_dictionary(column, public=None, group=None, ctx=None, device=None,
                            stream=None, max_distinct: Optional[int] = None) -> StringDictionary:
    """Global dense ids for a StringColumn of partition keys, the same on every
    rank, and every rank's slice of the string table
    (ColumnarData(global_string_keys=True)).

    column: this rank's StringColumn; public: the public partitions as a list
    of str, the same on every rank, or None.  group: the process group; None =
    one process (R = 1, no collective).  Device path: `ctx` (the library
    context) and `device`; without a context the column is taken on the host
    and numpy restatements of the kernels run the same protocol (the gloo CPU
    tests), as build_key_dictionary does.

    1. Local, as string_columns.encode_partition_keys: dpg_string_hash (through
       string_columns.device_keys), dpg_keydict_insert_slots into a table sized
       by `max_distinct` (else by n), dpg_keydict_representatives,
       dpg_string_verify, and ONE host synchronisation reading the distinct
       count D, the invalid-offset, lost and local mismatch counts.  Nothing
       is raised yet: a rank with errors runs every step below with what it
       has (a record with invalid offsets or without a slot reads nothing).
    2. Ids: the D distinct hashes and the hashes of the public strings (the
       column's hash_seed) go through build_key_dictionary unchanged: owner
       key_owner(hash, R), global id i * R + owner with i the hash's ascending
       signed rank among the owner's hashes, P, owned_keys, public_ids.  The
       ids are scattered to the occupied slots (the representatives' array is
       reused) and dpg_keydict_gather_ids gives every record its id: 4 B in,
       8 B out per record, no second probe.
    3. Strings to owners: the D representative strings, ordered by owner, are
       packed (dpg_string_lengths, a cumsum over D entries, dpg_string_pack:
       string_columns.pack_strings) and travel with their hashes and lengths:
       two `_split_sizes` all_gathers (strings, bytes; a byte or string total
       of 2^31 or more on any rank raises the same ValueError everywhere) and
       three all_to_all_single.  The public strings this rank owns are packed
       from the public column by the same call and join the arrivals as one
       more source; they are not sent.
    4. At the owner: the arrivals are sorted by hash with their index as
       payload (dpg_sort_pairs_u64 on key ^ 2^63; stable, so a run is in
       source-rank order), dpg_string_verify_runs compares every arrival with
       its predecessor in the run -- this is where two different strings of
       two ranks with one hash meet -- and the heads are packed once more, in
       owned_keys order, into the owned string table (owned_offsets,
       owned_data; on the device).
    5. ONE all_reduce (sum) of [invalid offsets, lost, local mismatches, owner
       mismatches, internal], after which every rank raises the same
       ValueError, in this order: invalid offsets, table overflow (naming
       max_distinct_partition_keys), "{k} records or strings share a 64-bit
       hash with a different string; pass another hash_seed" with k = local +
       owner mismatches; then RuntimeError when any owner's head count is not
       len(owned_keys) (internal).

    Collectives with R > 1, run by every rank whatever it holds: the four of
    build_key_dictionary, two all_gathers, three all_to_all_single and one
    all_reduce -- ten.  Host synchronisations on the device path: one in step
    1, three in build_key_dictionary's (its count and split, its lookup
    check), the split counts and one byte total per packed column (sent,
    public, owned) and the head count.

    The ids depend only on the union of the string sets, the seed and R.  With
    R = 1 they are the ascending signed rank of the hashes -- NOT the rank of
    the sorted strings that string_columns.encode_partition_keys (the default
    one-process route) gives."""
    world = 1 if group is None else dist.get_world_size(group)
    rank = 0 if group is None else dist.get_rank(group)
    on_device = ctx is not None and device is not None and torch.device(device).type == "cuda"
    dev = torch.device(device) if on_device else torch.device("cpu")
    kctx = ctx if on_device else None
    sptr = stream
    if on_device and sptr is None:
        sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # ---- 1. local
    offsets, data, hashes, rep_rec, finish, errs = _local_string_keys(
        column, dev, kctx, sptr, max_distinct)
    D = int(hashes.numel())
    # ---- 2. ids
    pub_col = pub_hash = None
    if public is not None:
        pub = string_columns.StringColumn.from_strings(public, column.encoding)
        if on_device:
            pub_col = pub.device_columns(dev)
            pub_hash, _ = string_columns.device_keys(*pub_col, column.hash_seed, ctx, sptr)
        else:
            pub_col = tuple(torch.from_numpy(x) for x in pub.host_columns())
            pub_hash = torch.from_numpy(string_columns.host_keys(
                *pub.host_columns(), column.hash_seed)[0])
    kd = build_key_dictionary(hashes, pub_hash, group, kctx, sptr)
    ids = finish(kd.ids)
    # ---- 3. strings to owners
    dest = key_owner(hashes, world)
    order = torch.argsort(dest, stable=True)
    s_off, s_data, _ = string_columns.pack_strings(offsets, data, rep_rec[order], kctx, sptr)
    s_hash = hashes[order]
    s_len = s_off[1:] - s_off[:-1]
    if world > 1:
        counts = torch.bincount(dest, minlength=world).cpu()  # a host synchronisation
        bounds = torch.cumsum(counts, 0)
        ends = s_off.cpu()[bounds]
        nbytes = ends - torch.cat([ends.new_zeros(1), ends[:-1]])
        in_n, out_n = _split_sizes(counts, group, dev, "string dictionary", "strings")
        in_b, out_b = _split_sizes(nbytes, group, dev, "string dictionary", "bytes of strings")
        a_hash = _exchange_column(s_hash, in_n, out_n, group)
        a_len = _exchange_column(s_len.contiguous(), in_n, out_n, group)
        a_data = _exchange_column(s_data, in_b, out_b, group)
    else:
        a_hash, a_len, a_data = s_hash, s_len, s_data
    del s_off, s_data, s_hash, s_len
    if pub_hash is not None:
        mine = torch.nonzero(key_owner(pub_hash, world) == rank).view(-1)
        p_off, p_data, _ = string_columns.pack_strings(*pub_col, mine, kctx, sptr)
        a_hash = torch.cat([a_hash, pub_hash[mine]])
        a_len = torch.cat([a_len, p_off[1:] - p_off[:-1]])
        a_data = torch.cat([a_data, p_data])
    M = int(a_hash.numel())
    a_off = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    torch.cumsum(a_len, 0, out=a_off[1:])
    # a sender's lengths and bytes come from one pack, so the offsets end at
    # the bytes; anything else is caught by the kernels' range checks
    # ---- 4. at the owner
    biased = (a_hash ^ _I64_MIN).contiguous()
    if on_device:
        idx = torch.arange(M, dtype=torch.int32, device=dev)
        srt = torch.empty_like(biased)
        srt_idx = torch.empty_like(idx)
        ctx.sort_pairs_u64(biased.data_ptr(), idx.data_ptr(), M, 0, 64, srt.data_ptr(),
                           srt_idx.data_ptr(), sptr)
    else:
        # unsigned order of key ^ 2^63 = signed order of the key
        o = torch.from_numpy(np.argsort(a_hash.numpy(), kind="stable"))
        srt, srt_idx = biased[o], o.to(torch.int32)
    head, owner_info = string_columns.verify_runs(srt, srt_idx, a_off, a_data, kctx, sptr)
    heads = srt_idx[torch.nonzero(head).view(-1)].to(torch.int64)  # a host synchronisation
    owned_offsets, owned_data, _ = string_columns.pack_strings(a_off, a_data, heads, kctx, sptr)
    n_owned = int(kd.owned_keys.numel())
    internal = int(heads.numel() != n_owned)
    # ---- 5. every rank's errors, summed
    t = torch.tensor(errs + [0, internal], dtype=torch.int64)
    t[3] = owner_info[:1].cpu()[0]
    if world > 1:
        t = t.to(_coll_device(group, dev))
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    invalid, lost, mismatch, owner_mismatch, internal = t.tolist()
    if invalid:
        raise ValueError(STRING_OFFSETS_ERROR.format(invalid))
    if lost:
        raise ValueError(STRING_OVERFLOW_ERROR.format(max_distinct, lost))
    if mismatch + owner_mismatch:
        raise ValueError(STRING_COLLISION_ERROR.format(mismatch + owner_mismatch))
    if internal:
        raise RuntimeError("string dictionary: an owner's distinct arrivals are not its owned "
                           "keys (internal error)")
    return StringDictionary(ids=ids, public_ids=kd.public_ids, n_partitions=kd.n_partitions,
                            owned_keys=kd.owned_keys, owned_offsets=owned_offsets,
                            owned_data=owned_data, encoding=column.encoding, ctx=kctx)


def place_records(enc, backend, mode: str) -> None:
    """ColumnarData(sharding=mode) with several ranks, applied to the encoded
    input `enc` in place before bounding or pre-aggregation: 'trusted' does
    nothing, 'verify' checks that this rank owns every privacy id it holds
    (one kernel, one all_reduce; every rank raises when any rank fails),
    'shuffle' sends every record to its owner (shuffle_records) and leaves
    what arrives, with record id offset 0.  Wide privacy ids (enc.pid_wide)
    are owned by `shard_of_wide`: the check and the split are the _wide calls."""
    if backend.world_size <= 1 or mode == "trusted":
        return
    if not enc.pid_unencoded:
        # the column's type is the same on every rank, so every rank raises
        raise ValueError(
            f"sharding={mode!r} needs integer privacy ids spanning at most 2^32 values: a "
            f"per-rank dictionary encoding of other ids is not consistent across ranks")
    dev, group = backend.device, backend.process_group
    with torch.cuda.device(dev):
        sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if mode == "verify":
            n_bad = torch.empty(1, dtype=torch.int64, device=dev)
            check = backend.ctx.check_shard_wide if enc.pid_wide else backend.ctx.check_shard
            check(ctypes.c_void_p(enc.pid.data_ptr()), enc.n, backend.world_size,
                  dist.get_rank(group), n_bad.data_ptr(), sptr)
            # no rank raises before the collective
            total = sum_over_ranks(n_bad, group)
            if total:
                raise ValueError(
                    f"sharding='verify': {total} records are on a rank that does not own "
                    f"their privacy id (distributed."
                    f"{'shard_of_wide' if enc.pid_wide else 'shard_of'}); use sharding='shuffle'")
            return
        enc.pid, enc.pk, enc.value = shuffle_records(enc.pid, enc.pk, enc.value, group,
                                                     backend.ctx, sptr, wide=enc.pid_wide)
    enc.n = int(enc.pk.numel())
    enc.rec_id_offset = 0
    if not enc.pid_range_declared:  # a declared range is global; else the device reduces it
        enc.pid_min, enc.pid_count = 0, 0


PID_DICT_ROUTES = ("slots", "lookup")
# The product route of `local_pid_dictionary`, chosen by the A/B of DESIGN.md
# section 17 (tools/bench_privacy_id_dictionary.py).
PID_DICT_ROUTE = "slots"


def _pid_capacity(n: int, max_distinct: Optional[int]) -> int:
    """Slots of the privacy-id table: the power of two >= 2 x min(n,
    max_distinct), in [64, 2^31] (the table calls' limit)."""
    bound = n if max_distinct is None else min(n, max(0, int(max_distinct)))
    return min(1 << 31, max(64, 1 << max(2 * bound - 1, 0).bit_length()))


def local_pid_dictionary(pid: torch.Tensor, ctx, stream, max_distinct: Optional[int] = None,
                         route: Optional[str] = None):
    """The device half of `encode_privacy_ids` up to the error check: returns
    (finish, D, n_reserved, n_lost) -- D distinct ids, the records holding the
    reserved id and the records that found no slot, read back together (the
    one host synchronisation) -- and `finish()`, which maps every record and
    returns the int64 ids: the ascending rank of each record's id among the D.

    route "slots": dpg_keydict_insert_slots remembers every record's slot and
    dpg_keydict_gather_ids reads the id there -- the table is probed once per
    record.  route "lookup": the composition of dpg_keydict_insert and
    dpg_keydict_lookup that `build_key_dictionary` uses, which probes twice.
    Both give the same ids; None takes PID_DICT_ROUTE."""
    route = PID_DICT_ROUTE if route is None else route
    if route not in PID_DICT_ROUTES:
        raise ValueError(f"unknown privacy-id dictionary route {route!r}")
    dev = pid.device
    n = pid.numel()
    capacity = _pid_capacity(n, max_distinct)
    slots = torch.full((capacity,), _I64_MIN, dtype=torch.int64, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    rec_slots = None
    if route == "slots":
        rec_slots = torch.empty(n, dtype=torch.int32, device=dev)  # uint32 bit patterns
        ctx.keydict_insert_slots(pid.data_ptr(), n, slots.data_ptr(), capacity,
                                 rec_slots.data_ptr(), info.data_ptr(), stream)
    else:
        ctx.keydict_insert(pid.data_ptr(), n, slots.data_ptr(), capacity, info.data_ptr(), stream)
    found = torch.empty(capacity, dtype=torch.int64, device=dev)
    n_found = torch.empty(1, dtype=torch.int64, device=dev)
    ctx.keydict_keys(slots.data_ptr(), capacity, found.data_ptr(), n_found.data_ptr(), stream)
    D, n_reserved, n_lost = torch.cat([n_found, info]).tolist()  # the one host synchronisation
    biased = found[:D] ^ _I64_MIN  # unsigned order of id ^ 2^63 = signed order of id
    distinct = torch.empty_like(biased)
    ctx.sort_pairs_u64(biased.data_ptr(), None, D, 0, 64, distinct.data_ptr(), None, stream)
    distinct ^= _I64_MIN
    del found, biased
    slot_ids = torch.empty(capacity, dtype=torch.int32, device=dev)
    n_missing = torch.zeros(1, dtype=torch.int64, device=dev)
    ranks = torch.arange(D, dtype=torch.int64, device=dev)
    ctx.keydict_assign(distinct.data_ptr(), ranks.data_ptr(), D, slots.data_ptr(),
                       slot_ids.data_ptr(), capacity, n_missing.data_ptr(), stream)

    def finish() -> torch.Tensor:
        # a record without an id is one that `info` counted, and the caller
        # has raised for those: n_missing is not read back
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        if route == "slots":
            ctx.keydict_gather_ids(rec_slots.data_ptr(), n, slot_ids.data_ptr(), capacity,
                                   ids.data_ptr(), n_missing.data_ptr(), stream)
        else:
            ctx.keydict_lookup(pid.data_ptr(), n, slots.data_ptr(), slot_ids.data_ptr(), capacity,
                               ids.data_ptr(), n_missing.data_ptr(), stream)
        return ids

    return finish, D, n_reserved, n_lost


def encode_privacy_ids(enc, backend) -> None:
    """ColumnarData(wide_privacy_ids=True): replaces the caller's int64 privacy
    ids in the encoded input `enc` (marked enc.pid_wide; else nothing happens)
    by dense ids, in place, right after `place_records` -- under "shuffle" on
    the received records.  Privacy ids never appear in a result and bounding
    is shard-local, so the dictionary is rank-local: the id of a privacy id is
    its ascending rank among this rank's distinct ids, exactly what
    torch.unique(return_inverse=True) -- the default encoding of one process
    -- gives.  No key travels.

    Device tensors (the library context backend.ctx): `local_pid_dictionary`,
    a write-once hash table of `_pid_capacity` slots (12 bytes per slot plus 8
    for the compaction, and 4 bytes per record for the remembered slots) with
    ONE host synchronisation, the read of the distinct count.  Host tensors
    (the gloo CPU tests): torch.unique, the reserved count and the table's
    capacity check mirrored.

    Errors are agreed on before anyone raises.  With several ranks ONE
    all_reduce (sum) carries each rank's records holding the reserved id
    INT64_MIN, its records that found no slot and its other local
    precondition failures (n >= 2^31, the table calls' limit); no rank raises
    between `place_records` and this collective, a rank without records runs
    it too, and after it every rank raises the same ValueError.  One process
    raises directly.  The ids of a StringColumn are its hashes
    (columnar.encode) and arrive here with the count of records whose offsets
    were invalid (enc.pid_bad_offsets), which travels in the same all_reduce."""
    if not enc.pid_wide:
        return
    world = backend.world_size
    group = backend.process_group if world > 1 else None
    pid = enc.pid.to(torch.int64).contiguous().view(-1)
    dev = pid.device
    n = pid.numel()
    max_distinct = enc.max_distinct_pids
    too_many = int(n >= 1 << 31)
    finish, D, n_reserved, n_lost = None, 0, 0, 0
    if too_many:
        pass
    elif dev.type == "cuda":
        with torch.cuda.device(dev):
            sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            finish, D, n_reserved, n_lost = local_pid_dictionary(pid, backend.ctx, sptr,
                                                                 max_distinct)
    else:
        uniq, inv = torch.unique(pid, return_inverse=True)
        n_reserved = int((pid == _I64_MIN).sum().item())
        D = int(uniq.numel())
        if max_distinct is not None:  # the device table's capacity, mirrored
            n_lost = max(0, D - _pid_capacity(n, max_distinct))
        finish = lambda: inv.to(torch.int64)
    bad_offsets = int(enc.pid_bad_offsets.item()) if enc.pid_bad_offsets is not None else 0
    if world > 1:
        t = torch.tensor([n_reserved, n_lost, too_many, bad_offsets], dtype=torch.int64,
                         device=_coll_device(group, dev))
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        n_reserved, n_lost, too_many, bad_offsets = t.tolist()
    if bad_offsets:
        raise ValueError(f"{bad_offsets} records of the privacy id StringColumn have offsets "
                         f"outside 0 <= offsets[i] <= offsets[i + 1] <= len(data)")
    if too_many:
        raise ValueError("wide privacy ids: a rank holds 2^31 or more records; the id "
                         "dictionary takes fewer")
    if n_reserved:
        raise ValueError(
            f"wide privacy ids: {n_reserved} records hold the privacy id INT64_MIN (-2^63), "
            f"which the id dictionary reserves")
    if n_lost:
        raise ValueError(
            f"wide privacy ids: the id dictionary sized by max_distinct_privacy_ids="
            f"{max_distinct} overflowed ({n_lost} records found no slot on their rank); raise "
            f"max_distinct_privacy_ids to at least the number of distinct privacy ids of one "
            f"rank")
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            enc.pid = finish()
    else:
        enc.pid = finish()
    enc.pid_min, enc.pid_count = 0, max(1, D)
    enc.pid_wide = False
    enc.pid_bad_offsets = None


def exchange_owner_pairs(pairs: torch.Tensor, n_pairs: int, P: int, group, ctx=None,
                         stream=None):
    """Delivers the entries of a pk-sorted pre-aggregate to the ranks that own
    their partitions and merges what arrives.

    pairs: float64 [cap, 3] tensor viewed as 24-byte dpg_pair_entry, the first
    n_pairs of them ascending by pk (as dpg_preaggregate writes them) with pk
    the global dense id in [0, P).  The entry of partition pk goes to rank
    pk % R and arrives with pk re-based to the owner's local id pk // R; its
    other 20 bytes travel unchanged.

    Returns (pairs, starts, n_local, n, n_bad): this rank's owned slice as a
    pre-aggregate -- the received entries ascending by local pk and, within a
    partition, by source rank and then by the source's order; starts
    (int64[n_local + 1]) delimiting the partitions; n_local =
    owned(P, R, rank)[2]; the number of entries n; and n_bad, a one-element
    int64 tensor counting received entries that were out of range or out of
    order (nonzero only if a sender broke the contract: such entries are
    dropped, and the caller is expected to fail on every rank).

    Device tensors with the library context `ctx`: ONE stable split on the
    device (dpg_owner_split_pairs) and one merge of the received runs
    (dpg_merge_pair_runs), stream-ordered on `stream` (torch's current
    stream); reading the split's R counts back is the exchange's one host
    synchronisation.  Host tensors (the gloo CPU tests, no context): the same
    layout from a stable argsort of pk % R and, for the merge, of the received
    local pk.

    Every rank runs the same collectives whatever it holds, nothing included:
    one all_gather of the R counts (`_split_sizes`: a receive total of 2^31 or
    more on any rank raises the same ValueError everywhere) and one
    all_to_all_single of the entries as float64 words (splits x 3).  The send
    buffer is freed before the merge."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = pairs.device
    n = int(n_pairs)
    n_local = owned(P, world, rank)[2]
    pairs = pairs.contiguous().view(-1, 3)
    on_device = ctx is not None and dev.type == "cuda"
    if on_device:
        send = torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev)
        counts = torch.empty(world, dtype=torch.int64, device=dev)
        ctx.owner_split_pairs(pairs.data_ptr(), n, world, send.data_ptr(), counts.data_ptr(),
                              stream)
        counts = counts.cpu()  # the one host synchronisation
        send = send[:n]
    else:
        send = pairs[:n].clone()
        pk = _pair_pk(send)
        dest = pk % world
        order = torch.argsort(dest, stable=True)
        counts = torch.bincount(dest, minlength=world).cpu()
        _set_pair_pk(send, pk // world)
        send = send[order]
    del pairs
    in_splits, out_splits = _split_sizes(counts, group, dev, "pair exchange", "pairs")
    recv = _exchange_column(send.reshape(-1), [3 * c for c in in_splits],
                            [3 * c for c in out_splits], group).view(-1, 3)
    del send
    total = sum(out_splits)
    if on_device:
        run_start = [0]
        for c in out_splits:
            run_start.append(run_start[-1] + c)
        merged = torch.empty((max(total, 1), 3), dtype=torch.float64, device=dev)
        starts = torch.empty(n_local + 1, dtype=torch.int64, device=dev)
        n_bad = torch.empty(1, dtype=torch.int64, device=dev)
        ctx.merge_pair_runs(recv.data_ptr(), run_start, n_local, merged.data_ptr(),
                            starts.data_ptr(), n_bad.data_ptr(), stream)
        return merged, starts, n_local, total, n_bad
    pk = _pair_pk(recv)
    run = torch.repeat_interleave(torch.arange(world), torch.tensor(out_splits))
    # bad as dpg_merge_pair_runs defines it: out of range, or below an
    # in-range predecessor of the same run
    prev_ok = torch.zeros(total, dtype=torch.bool)
    if total > 1:
        prev_ok[1:] = (run[1:] == run[:-1]) & (pk[:-1] < n_local)
    bad = pk >= n_local
    if total > 1:
        bad[1:] |= prev_ok[1:] & (pk[1:] < pk[:-1])
    keep = torch.nonzero(~bad).flatten()
    order = keep[torch.argsort(pk[keep], stable=True)]
    merged = recv[order]
    starts = torch.searchsorted(pk[order].contiguous(), torch.arange(n_local + 1))
    return (merged.to(dev), starts.to(torch.int64).to(dev), n_local, int(order.numel()),
            bad.sum().reshape(1).to(torch.int64).to(dev))


def _pair_pk(pairs: torch.Tensor) -> torch.Tensor:
    """pk (the first 32-bit word, unsigned) of float64 [n, 3] pair entries."""
    return pairs.view(torch.int32).view(-1, 6)[:, 0].to(torch.int64) & 0xFFFFFFFF


def _set_pair_pk(pairs: torch.Tensor, pk: torch.Tensor) -> None:
    words = pairs.view(torch.int32).view(-1, 6)
    words[:, 0] = torch.where(pk >= 1 << 31, pk - (1 << 32), pk).to(torch.int32)


def _names(tensors) -> list:
    return [k for k in _PACK_ORDER if tensors.get(k) is not None]


def _interleaved(t: torch.Tensor, P: int, world: int, S: int) -> torch.Tensor:
    """[world, S] float64 view of partition array t: element (r, i) is
    partition i * world + r (zero past P)."""
    x = torch.zeros(S * world, dtype=torch.float64, device=t.device)
    x[:P] = t.to(torch.float64)
    return x.view(S, world).t()


def _unpack_column(col: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return (col.round().to(torch.int64) if like.dtype == torch.int64 else col).contiguous()


def reduce_scatter_partials(tensors: Dict[str, Optional[torch.Tensor]], P: int, group,
                            err: Optional[torch.Tensor] = None, ctx=None, stream=None):
    """Sums the dense partials over ranks; returns this rank's partitions
    of every array, (lo, stride, n) and the summed error flags (a [1]
    float64 tensor on the partials' device), with one collective for all
    of them.  Layout [rank][array][S] + one error slot per rank block --
    the C ABI's dpg_pack_partials layout.

    Device partials with the library context `ctx` (the product path): ONE
    pack kernel (dpg_pack_partials: every array interleaved into its rank
    blocks, int64 -> float64, zero past P, the context's error flag in each
    block's last slot) and ONE unpack kernel (dpg_unpack_partials: this
    rank's block back into int64 / float64 slices, a nonzero error sum
    latched for dpg_compact_kept), stream-ordered on `stream` (torch's
    current stream, which the collective waits on) -- one pass over the
    partials each way.  Host partials (the gloo CPU tests, no context): the
    same layout built with torch ops."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    S = (P + world - 1) // world
    lo, stride, n_local = owned(P, world, rank)
    names = _names(tensors)
    A = len(names)
    dev = tensors[names[0]].device
    # the library's pack / unpack kernels read and write the partials
    # through raw pointers: only contiguous arrays of the layout they assume
    # (int64 rows / count, float64 sums) take them; anything else takes the
    # torch path, which handles any dtype
    fused = (ctx is not None and dev.type == "cuda" and
             all(tensors[k].is_contiguous() and tensors[k].dtype == _PACK_DTYPE[k]
                 and tensors[k].numel() >= P for k in names))
    pack = torch.empty((world, A * S + 1), dtype=torch.float64, device=dev)
    if fused:
        from pipelinedp_amd import _native
        full = _native.Partials(P, *(tensors[k].data_ptr() if tensors.get(k) is not None else None
                                     for k in _PACK_ORDER))
        ctx.pack_partials(full, world, pack.data_ptr(), stream)
    else:
        for j, k in enumerate(names):
            pack[:, j * S:(j + 1) * S] = _interleaved(tensors[k], P, world, S)
        pack[:, A * S] = err.to(dev).reshape(()) if err is not None else 0.0
    if _is_nccl(group):
        part = torch.empty(A * S + 1, dtype=torch.float64, device=dev)
        dist.reduce_scatter_tensor(part, pack.view(-1), op=dist.ReduceOp.SUM, group=group)
    else:
        host = pack.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        part = host[rank].to(dev)
    del pack
    out: Dict[str, Optional[torch.Tensor]] = {k: None for k in _PACK_ORDER}
    if fused:
        from pipelinedp_amd import _native
        for k in names:
            out[k] = torch.empty(max(n_local, 1), dtype=tensors[k].dtype, device=dev)
        sl = _native.Partials(n_local, *(out[k].data_ptr() if out.get(k) is not None else None
                                         for k in _PACK_ORDER))
        lo_k, n_k = ctx.unpack_partials(part.data_ptr(), P, world, rank, sl, stream)
        assert (lo_k, n_k) == (lo, n_local), (lo_k, n_k, lo, n_local)
        for k in names:
            out[k] = out[k][:n_local]
    else:
        for j, k in enumerate(names):
            out[k] = _unpack_column(part[j * S:j * S + n_local], tensors[k])
    return out, (lo, stride, n_local), part[A * S:A * S + 1]


def occupancy_bound(P: int, n_records: int, pid_count: int, l0: int) -> int:
    """Upper bound on the partitions one rank's kept pairs can reach: at
    most one per record, at most l0 per privacy id, at most P."""
    b = min(P, max(0, n_records))
    if pid_count > 0 and l0 > 0:
        b = min(b, pid_count * l0)
    return max(1, b)


def exchange_bytes(P: int, nnz_bound: int, n_arrays: int, world: int = 1) -> Dict[str, int]:
    """Bytes one rank sends in each exchange."""
    S = (P + world - 1) // world
    cap = min(S, nnz_bound)
    return {"reduce_scatter": 8 * world * (n_arrays * S + 1),
            "all_to_all": 8 * world * (cap + 1) * (1 + n_arrays)}


def choose_exchange(P: int, n_arrays: int, world: int, nnz_bound: int, mode: str = "auto") -> str:
    """The exchange of one release, from sizes every rank agrees on (no
    device data): 'auto' takes the sparse all-to-all when its fixed blocks
    are at most half the dense reduce-scatter's bytes."""
    if mode not in ("auto", "reduce_scatter", "all_to_all"):
        raise ValueError(f"unknown exchange {mode!r}")
    if mode != "auto":
        return mode
    b = exchange_bytes(P, nnz_bound, n_arrays, world)
    return "all_to_all" if 2 * b["all_to_all"] <= b["reduce_scatter"] else "reduce_scatter"


def all_to_all_partials(tensors: Dict[str, Optional[torch.Tensor]], P: int, group,
                        nnz_bound: int, err: Optional[torch.Tensor] = None):
    """Sparse merge: the occupied partitions (rows > 0) of every rank travel
    as (pk, partials...) rows to their owner in fixed blocks of cap rows per
    destination (equal splits: nothing about the occupancy reaches the
    host).  The owner adds them into its dense slice source rank by source
    rank (pks are unique within one source, so every add is conflict-free
    and the merge is deterministic).  Same result as
    reduce_scatter_partials.  A block with more occupied partitions than cap
    (impossible when nnz_bound bounds the occupancy) raises the error flag.

    The send side works on the occupied partitions only: at most K =
    min(P, nnz_bound) of them, taken by one fixed-size nonzero (no host
    sync), ordered by owner with a stable sort, so its temporaries are
    K-sized (the sparse exchange is chosen exactly when K is far below P
    / R: ADVICE r4)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    S = (P + world - 1) // world
    cap = max(1, min(S, int(nnz_bound)))
    lo, stride, n_local = owned(P, world, rank)
    names = _names(tensors)
    A = len(names)
    dev = tensors[names[0]].device
    K = max(1, min(P, int(nnz_bound)))
    occ = tensors["rows"] > 0
    n_occ = occ.sum()
    idx = torch.nonzero_static(occ, size=K, fill_value=P).view(-1)   # ascending, pad P
    valid = idx < P
    own = torch.where(valid, idx % world, torch.full_like(idx, world))
    order = torch.argsort(own, stable=True)                          # by owner, pk ascending
    idx, own, valid = idx[order], own[order], valid[order]
    cnt = torch.bincount(own, minlength=world + 1)
    start = torch.cumsum(cnt, 0) - cnt
    pos = torch.arange(K, device=dev) - start[own]
    fits = valid & (pos < cap)
    over = ((n_occ > K) | (valid & ~fits).any()).to(torch.float64)
    blk = cap + 1                                                  # header row + cap rows
    sink = world * blk                                             # rows past the cap, padding
    dst = torch.where(fits, own * blk + 1 + pos, torch.full_like(pos, sink))
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    rows = torch.stack([idx.to(torch.float64)] +
                       [tensors[k][safe].to(torch.float64) for k in names], -1)
    send = torch.zeros((sink + 1, 1 + A), dtype=torch.float64, device=dev)
    send[:, 0] = -1.0
    send.index_copy_(0, dst, rows)
    hdr = torch.arange(world, device=dev) * blk
    send[hdr, 0] = -2.0
    send[hdr, 1] = (err.to(dev).reshape(()) if err is not None else 0.0) + over
    send = send[:sink].contiguous()
    nccl = _is_nccl(group)
    if nccl:
        recv = torch.empty_like(send)
        dist.all_to_all_single(recv, send, group=group)
    else:
        recv = torch.empty_like(send, device="cpu")
        dist.all_to_all_single(recv, send.cpu(), group=group)
        recv = recv.to(dev)
    recv = recv.view(world, blk, 1 + A)
    flags = recv[:, 0, 1].sum().reshape(1)
    acc = torch.zeros((A, n_local + 1), dtype=torch.float64, device=dev)
    for src in range(world):  # source rank order: deterministic sums
        body = recv[src, 1:]
        pk = body[:, 0]
        li = torch.where(pk >= 0, (pk.round().to(torch.int64) - lo) // stride,
                         torch.full_like(pk, n_local, dtype=torch.int64))
        acc.index_add_(1, li, body[:, 1:].t().contiguous())
    out: Dict[str, Optional[torch.Tensor]] = {k: None for k in _PACK_ORDER}
    for j, k in enumerate(names):
        out[k] = _unpack_column(acc[j, :n_local], tensors[k])
    return out, (lo, stride, n_local), flags


def exchange_partials(tensors: Dict[str, Optional[torch.Tensor]], P: int, group,
                      mode: str = "auto", nnz_bound: Optional[int] = None,
                      err: Optional[torch.Tensor] = None, ctx=None, stream=None):
    """Merges the partials of every rank into this rank's partitions with
    the exchange `choose_exchange` picks.  nnz_bound must be the same on
    every rank (release_header); None = P.  ctx / stream: the library
    context and its stream, for the fused pack / unpack kernels of the
    dense exchange.  Returns (tensors, (lo, stride, n), info, error flags)
    where info names the exchange and its per-rank send bytes."""
    names = _names(tensors)
    world = dist.get_world_size(group)
    bound = P if nnz_bound is None else int(nnz_bound)
    chosen = choose_exchange(P, len(names), world, bound, mode)
    if chosen == "all_to_all":
        out, own, flags = all_to_all_partials(tensors, P, group, bound, err)
    else:
        out, own, flags = reduce_scatter_partials(tensors, P, group, err, ctx, stream)
    info = {"mode": chosen, "backend": dist.get_backend(group), "world_size": world,
            "nnz_bound": bound,
            "send_bytes": exchange_bytes(P, bound, len(names), world)[chosen]}
    return out, own, info, flags


def _all_reduce(t: torch.Tensor, op, group) -> torch.Tensor:
    """all_reduce of t on its device under nccl, staged through the host
    under gloo; the result on t's device."""
    if _is_nccl(group) or t.device.type == "cpu":
        dist.all_reduce(t, op=op, group=group)
        return t
    host = t.cpu()
    dist.all_reduce(host, op=op, group=group)
    return host.to(t.device)


def hist_header(sum_range: torch.Tensor, n_bound: int, group):
    """ONE all_reduce (max) before the dataset histograms' exchange, of
    [-min, max, n_bound] as float64: the range of the pair sums over all ranks
    (negating the min is exact; a rank without pairs holds (+inf, -inf) and
    changes nothing) and the largest per-rank occupancy bound, which every
    rank then passes to `choose_exchange`.  sum_range: float64[2] (min, max).
    Returns (range, bound): the float64[2] range of the whole dataset on
    sum_range's device -- (+inf, -inf) if no rank has a pair -- and the bound
    as an int; reading it synchronises the host."""
    t = torch.stack([-sum_range[0], sum_range[1],
                     torch.tensor(float(n_bound), dtype=torch.float64,
                                  device=sum_range.device)])
    t = _all_reduce(t, dist.ReduceOp.MAX, group)
    return torch.stack([-t[0], t[1]]), int(t[2].item())


_KEY_FLIP = (1 << 63) - 1


def _ordered_keys(b: torch.Tensor) -> torch.Tensor:
    """The bit patterns (int64) of float64 values -> int64 keys whose signed
    order is the values' order, and back: the map is its own inverse."""
    return torch.where(b >= 0, b, b ^ _KEY_FLIP)


def merge_histograms(int_bins: torch.Tensor, sum_count: torch.Tensor, sum_sum: torch.Tensor,
                     sum_max: torch.Tensor, flags: Optional[torch.Tensor], group):
    """Merges every rank's histogram bins into the bins of the whole dataset,
    the same on every rank, with THREE collectives:

    * one int64 SUM: the counts and sums of the integer bins
      (int_bins[..., 0:2]; int64 [T, bins, 3]: count, sum, max), the LINF_SUM
      counts and one slot of error flags (`flags`: any tensor, e.g. the
      exchange's, nonzero = this rank saw an error);
    * one int64 MAX: the integer maxima (int_bins[..., 2]) and the LINF_SUM
      maxima as order-preserving integer keys, INT64_MIN where this rank's
      bin is empty (a float maximum of 0.0 there would beat negative sums);
    * one float64 SUM: the LINF_SUM sums.

    Every rank runs all three whatever it holds.  A nonzero flag total raises
    RuntimeError on every rank, after the collectives.  Returns (int_bins,
    sum_count, sum_sum, sum_max) on the inputs' device; sum_max is 0.0 in a
    bin that is empty on every rank."""
    T, nb, _ = int_bins.shape
    ns = sum_count.numel()
    dev = int_bins.device
    bad = (torch.zeros(1, dtype=torch.int64, device=dev) if flags is None
           else (flags.to(dev) != 0).sum().reshape(1).to(torch.int64))
    adds = torch.cat([int_bins[:, :, 0:2].reshape(-1), sum_count.reshape(-1), bad])
    keys = torch.where(sum_count > 0, _ordered_keys(sum_max.contiguous().view(torch.int64)),
                       torch.full_like(sum_count, _I64_MIN))
    maxes = torch.cat([int_bins[:, :, 2].reshape(-1), keys])
    adds = _all_reduce(adds, dist.ReduceOp.SUM, group)
    maxes = _all_reduce(maxes, dist.ReduceOp.MAX, group)
    sums = _all_reduce(sum_sum.clone(), dist.ReduceOp.SUM, group)
    n_bad = int(adds[-1].item())
    if n_bad:
        raise RuntimeError(f"dataset histograms: {n_bad} ranks reported an error in the "
                           f"exchange of the per-partition totals")
    merged = torch.empty_like(int_bins)
    merged[:, :, 0:2] = adds[:T * nb * 2].view(T, nb, 2)
    merged[:, :, 2] = maxes[:T * nb].view(T, nb)
    count = adds[T * nb * 2:T * nb * 2 + ns].contiguous()
    k = maxes[T * nb:]
    top = torch.where(count > 0, _ordered_keys(k), torch.zeros_like(k)).view(torch.float64)
    return merged, count, sums, top


def broadcast_object(obj, group, device):
    """Rank 0's (small, picklable) object on every rank: one object collective."""
    root = dist.get_global_rank(group, 0) if group is not None else 0
    box = [obj if dist.get_rank() == root else None]
    dist.broadcast_object_list(box, src=root, group=group,
                               device=device if _is_nccl(group) else None)
    return box[0]


def slice_bitmap(mask: torch.Tensor, lo: int, stride: int, n: int) -> torch.Tensor:
    """Bitmap of partitions lo + i * stride (i < n) re-based to bit i."""
    ids = lo + torch.arange(n, device=mask.device) * stride
    bits = ((mask[ids >> 3].to(torch.int64) >> (ids & 7)) & 1).to(torch.uint8)
    padded = torch.zeros(((n + 7) // 8) * 8, dtype=torch.uint8, device=mask.device)
    padded[:n] = bits
    weights = (1 << torch.arange(8, device=mask.device)).to(torch.int64)
    return (padded.view(-1, 8).to(torch.int64) * weights).sum(1).to(torch.uint8)


def all_gather_strings(out_offsets: torch.Tensor, out_data: torch.Tensor, sizes, group,
                       encoding: str = "utf-8") -> list:
    """Every rank's kept strings (a packed column: offsets int64[K + 1] and
    bytes) as one list of str in rank order, the same on every rank: ONE
    all_gather of the lengths, padded to the largest of `sizes` (every rank's
    K, as all_gather_results exchanged them), and ONE of the bytes, padded to
    the largest byte total, which the lengths give."""
    world = dist.get_world_size(group)
    cdev = _coll_device(group, out_offsets.device)
    m = max(sizes) if sizes else 0
    k = out_offsets.numel() - 1
    mine = torch.zeros(m, dtype=torch.int64, device=cdev)
    mine[:k] = (out_offsets[1:] - out_offsets[:-1]).to(cdev)
    lens = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(lens, mine, group=group)
    lens = [ln[:s].cpu() for ln, s in zip(lens, sizes)]
    totals = [int(ln.sum().item()) for ln in lens]
    buf = torch.zeros(max(totals) if totals else 0, dtype=torch.uint8, device=cdev)
    buf[:out_data.numel()] = out_data.to(cdev)
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf, group=group)
    out = []
    for ln, p, t in zip(lens, parts, totals):
        off = torch.zeros(ln.numel() + 1, dtype=torch.int64)
        torch.cumsum(ln, 0, out=off[1:])
        out += string_columns.decode_packed(off, p[:t], encoding)
    return out


def all_gather_results(ids: torch.Tensor, vals: torch.Tensor, group, exact_ids: bool = False,
                       return_sizes: bool = False):
    """Concatenates every rank's kept (ids, values) in rank order: one size
    exchange, then one all_gather of ids and values packed as float64 rows
    (ids < 2^53 are exact).  exact_ids: the ids are the caller's sparse int64
    keys, which a float64 does not hold: they travel in an int64 all_gather of
    their own.  return_sizes: every rank's kept count is returned as a third
    value (a list).  Runs after dpg_compact_kept, which has already
    synchronised the host."""
    world = dist.get_world_size(group)
    dev = ids.device
    cdev = _coll_device(group, dev)
    n = torch.tensor([ids.numel()], dtype=torch.int64, device=cdev)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(s.item()) for s in sizes]
    m = max(sizes) if sizes else 0
    cols = vals.shape[1] if vals.dim() == 2 else 0
    buf = torch.zeros((m, 1 + cols), dtype=torch.float64, device=cdev)
    buf[:ids.numel(), 0] = ids.to(torch.float64).to(cdev)
    if cols:
        buf[:ids.numel(), 1:] = vals.to(cdev)
    got = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(got, buf, group=group)
    rows = torch.cat([g[:s] for g, s in zip(got, sizes)]).to(dev)
    if exact_ids:
        mine = torch.zeros(m, dtype=torch.int64, device=cdev)
        mine[:ids.numel()] = ids.to(cdev)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        keys = torch.cat([p[:s] for p, s in zip(parts, sizes)]).to(dev)
        out = (keys, rows[:, 1:].to(vals.dtype).contiguous())
    else:
        out = (rows[:, 0].round().to(torch.int64), rows[:, 1:].to(vals.dtype).contiguous())
    return out + (sizes,) if return_sizes else out
