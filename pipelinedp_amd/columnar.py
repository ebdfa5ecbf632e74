"""Ingest: turn the user's collection into device columns for the kernels.

The reference extracts `(privacy_id, partition_key, value)` per row with the
DataExtractors callables (dp_engine.py:384-397).  The MI355X path keeps the
same extractors but prefers columnar input:

* `ColumnarData` / a mapping of columns (numpy arrays or torch tensors,
  ideally already on the GPU).  An extractor is then a column name or a
  callable applied to the whole container.
* Any other iterable is treated as rows; the extractors run per row on the
  host (reference behaviour, slow, meant for small inputs).

Keys: the kernels need integer privacy ids spanning at most 2^32 values and
dense partition ids in [0, P).  Integer keys that already satisfy this are
used as they are; anything else (strings, tuples, ints spread wider) is
dictionary-encoded (`unique` + inverse), and the partition dictionary maps
results back.  Encoding is ingest, not part of the DP computation.
ColumnarData(wide_privacy_ids=True) leaves int64 privacy ids of any span as
they are; the device numbers them after the records are placed
(distributed.encode_privacy_ids).  A StringColumn (string_columns.py: offsets
and bytes) is hashed on the device: as `pk` it gets the dense ids and the
key table a list of the same strings would get, as `pid` it becomes wide
privacy ids.
"""
import dataclasses
from collections.abc import Mapping
from typing import Any, Optional, Sequence, Tuple

import numpy as np
import torch

from . import string_columns
from .string_columns import StringColumn

_PID_SPAN = 1 << 32  # privacy ids of one call must span at most 2^32 values
SHARDING_MODES = ("trusted", "verify", "shuffle")


@dataclasses.dataclass
class ColumnarData:
    """Columnar collection for DPEngine.aggregate on the MI355X backend.

    `pid`, `pk`, `value`: torch tensors, numpy arrays or lists.  A column may
    be any strided view on any device (`table[:, j]`, `buf[1:]`, `x[::2]`):
    the encoder makes it a contiguous device column, copying only when it is
    not one already.  Integer columns of any width are widened to int64, float
    columns converted to float64; a scalar-metric `value` may be [n] or
    [n, 1].  The lengths must agree: a `pid` or `value` whose length differs
    from `pk`'s raises ValueError on the host.

    `n_partitions`: if given, `pk` must already hold dense ids in
    [0, n_partitions) and is passed to the device unchecked (the kernel still
    rejects out-of-range keys with ValueError).

    `privacy_id_range`: optional (lo, hi) with every privacy id in [lo, hi),
    hi - lo <= 2^32; saves the device a min/max pass (out-of-range ids raise
    ValueError).  `record_id_offset`: global id of record 0 -- the record
    sampler is keyed by (pid, pk, record id), so the shards of one dataset,
    each given its offset, sample exactly like the whole.

    `sharding` (several ranks only; see pipelinedp_amd.distributed): how this
    rank's records relate to the privacy-id shards.  "trusted": the caller
    put every privacy id on rank distributed.shard_of(pid, R), unchecked;
    "verify": the same claim, checked on the device (every rank raises
    ValueError if any rank holds a record it does not own); "shuffle": the
    records are split any way at all and are exchanged before bounding
    (record_id_offset is then ignored; a privacy_id_range must be global).
    "verify" and "shuffle" need integer privacy ids.

    `sparse_partition_keys` (opt-in): `pk` holds any int64 values but
    INT64_MIN -- hashes, timestamps, product ids -- and the device builds the
    dictionary that gives them dense ids, the same on every rank
    (distributed.build_key_dictionary).  This is how
    several ranks take keys that are not dense ids; one process runs the same
    kernels.  `pk` and the public partitions must then be integers, the public
    partitions the same on every rank, and `n_partitions` must not be given.
    Results carry the caller's keys.  `max_distinct_partition_keys`: an upper
    bound on one rank's distinct partition keys, public ones included, which
    sizes the hash table (else the record count does); a bound that is too
    small raises ValueError on every rank.

    `wide_privacy_ids` (opt-in): `pid` holds any int64 values but INT64_MIN --
    hashed user ids, half a UUID, tenant << 32 | user -- however wide they
    span.  The device gives them dense ids in a rank-local hash dictionary
    (distributed.encode_privacy_ids): the id of a
    privacy id is its ascending rank among the rank's distinct ids, which is
    what the default encoding of one process gives, without its sorts of the
    record column.  It works with and without `n_partitions`, with
    `sparse_partition_keys` and under every `sharding` mode; the owner of a
    privacy id is then distributed.shard_of_wide(pid, R), a hash of all 64
    bits, so a caller who pre-shards for "trusted" uses that.  `pid` must be an
    integer tensor or array (TypeError otherwise) and `privacy_id_range` must
    not be given.  `max_distinct_privacy_ids`: an upper bound on one rank's
    distinct privacy ids, which sizes the hash table (else the record count
    does); a bound that is too small raises ValueError on every rank.  With
    contribution_bounds_already_enforced the privacy ids are not read and the
    flag does nothing.

    String columns (opt-in): `pid` and `pk` may each be a StringColumn --
    Arrow's offsets + bytes layout, ideally already on the GPU -- which the
    device hashes to 64-bit keys; lists and arrays of
    `str` keep the host encoding.  A string `pk` is dictionary-encoded on the
    device, every record compared with the first record of its hash-table slot,
    so a hash collision raises ValueError ("pass another hash_seed") instead of
    merging two partitions; results carry the strings, and the public
    partitions are then a list or tuple of `str` or a StringColumn.
    `max_distinct_partition_keys` sizes its table too.  It runs in one process
    (several ranks: NotImplementedError) and excludes `n_partitions` and
    `sparse_partition_keys` (ValueError).  A string `pid` becomes wide privacy
    ids -- the hashes -- with everything said above about them, on one rank or
    several; a caller who pre-shards for "trusted" uses
    distributed.shard_of_wide(distributed.string_key_hash(column), R).
    `privacy_id_range` must not be given (ValueError).

    `global_string_keys` (opt-in): a string `pk` gets its ids from a global
    string dictionary (distributed.build_string_dictionary; DESIGN.md section
    19), on one rank or several, under every `sharding` mode and with integer,
    wide or string privacy ids.  Every rank hashes and verifies its own
    strings as above; the distinct hashes get global ids i * R + owner from
    the key dictionary of `sparse_partition_keys`; one representative string
    per hash travels to the hash's owner, which compares the strings that
    arrive under one hash -- so two different strings with one hash on
    DIFFERENT ranks raise the same ValueError on every rank -- and keeps its
    slice of the string table on the device.  With several ranks that is ten
    collectives before the records are placed.  Only the strings of the KEPT
    partitions are decoded on the host; results carry `str` keys, after a
    gather the same list on every rank.  The ids are the ascending rank of the
    hashes, not of the sorted strings as without the flag, so under binding
    bounds or with noise a flagged release draws other samples than the
    unflagged release of the same data (both are correct releases).  `pk` must
    be a StringColumn (ValueError otherwise); `n_partitions` and
    `sparse_partition_keys` stay excluded; `max_distinct_partition_keys` sizes
    the local table; the public partitions are a list or tuple of `str` or a
    StringColumn, the same on every rank.  Supported: aggregate with COUNT,
    SUM, PRIVACY_ID_COUNT, MEAN and VARIANCE, and select_partitions;
    PERCENTILE, VECTOR_SUM and the analysis, histogram and tune entry points
    raise NotImplementedError."""
    pid: Any = None
    pk: Any = None
    value: Any = None
    n_partitions: Optional[int] = None
    privacy_id_range: Optional[Tuple[int, int]] = None
    record_id_offset: int = 0
    sharding: str = "trusted"
    sparse_partition_keys: bool = False
    max_distinct_partition_keys: Optional[int] = None
    wide_privacy_ids: bool = False
    max_distinct_privacy_ids: Optional[int] = None
    global_string_keys: bool = False

    def __post_init__(self):
        if self.global_string_keys and not isinstance(self.pk, StringColumn):
            raise ValueError("global_string_keys=True builds a global string dictionary: pk "
                             "must be a StringColumn")
        if self.sharding not in SHARDING_MODES:
            raise ValueError(f"sharding must be one of {SHARDING_MODES}, got {self.sharding!r}")
        if self.sparse_partition_keys and self.n_partitions is not None:
            raise ValueError("sparse_partition_keys=True builds the dense partition ids itself: "
                             "n_partitions must not be given")
        if self.wide_privacy_ids:
            if self.privacy_id_range is not None:
                raise ValueError("wide_privacy_ids=True encodes the privacy ids itself: "
                                 "privacy_id_range must not be given")
            if self.pid is not None and not isinstance(self.pid, StringColumn):
                _check_wide_pid(self.pid)
        _check_string_columns(self.pid, self.pk, self.n_partitions, self.sparse_partition_keys,
                              self.privacy_id_range)

    def __getitem__(self, name):
        return getattr(self, name)

    def __len__(self):
        return len(self.pk)

    def __bool__(self):
        return self.pk is not None and len(self.pk) > 0


@dataclasses.dataclass
class EncodedInput:
    pid: Optional[torch.Tensor]
    pk: torch.Tensor
    value: Optional[torch.Tensor]
    n: int
    n_partitions: int
    key_table: Optional[Sequence]  # dense id -> original key (None: identity)
    public_mask: Optional[torch.Tensor] = None  # uint8 bitmap on the device
    public_count: int = 0
    pid_min: int = 0
    pid_count: int = 0        # 0: unknown (the device reduces min / max)
    rec_id_offset: int = 0
    partitions_declared: bool = False  # dense ids in [0, n_partitions) given by the caller
    # the privacy ids are the caller's integers, not a per-call dictionary
    # encoding (which differs from rank to rank): shard_of(pid) is global
    pid_unencoded: bool = False
    pid_range_declared: bool = False  # pid_min / pid_count come from privacy_id_range
    # sparse_partition_keys: pk still holds the caller's int64 keys (and
    # public_keys the public ones) until distributed.build_key_dictionary
    # replaces them by global dense ids
    pk_sparse: bool = False
    public_keys: Optional[torch.Tensor] = None
    # wide_privacy_ids: pid still holds the caller's int64 values (pid_min =
    # pid_count = 0) until distributed.encode_privacy_ids replaces them by the
    # rank's dense ids; max_distinct_pids sizes its table
    pid_wide: bool = False
    max_distinct_pids: Optional[int] = None
    # a StringColumn of privacy ids: pid holds its hashes (pid_wide) and this
    # device int64[1] the records whose offsets were invalid, which
    # distributed.encode_privacy_ids raises for on every rank alike
    pid_bad_offsets: Optional[torch.Tensor] = None
    # global_string_keys: the distributed.StringDictionary whose ids pk holds
    # (this rank's slice of the string table; the results' keys come from it)
    string_dictionary: Any = None


def _extract(col, extractor):
    if extractor is None:
        return None
    if isinstance(extractor, str):
        return col[extractor]
    return extractor(col)


def _is_columnar(col) -> bool:
    return isinstance(col, (ColumnarData, Mapping))


def _to_tensor(x, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device) if x.device != device else x
    a = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _length(x) -> int:
    try:
        return len(x)
    except TypeError:
        return int(np.asarray(x).shape[0])


def _check_length(name: str, x, n: int) -> None:
    """A column shorter than pk would be read past its end by the kernels
    (they take n = len(pk) and raw pointers); a longer one is a caller error
    too.  Host only: nothing is copied or launched before this."""
    m = _length(x)
    if m != n:
        raise ValueError(f"column {name} has {m} elements but pk has {n}: "
                         f"the columns of one collection must have the same length")


def _integer_like(x) -> bool:
    if isinstance(x, torch.Tensor):
        return not x.is_floating_point() and not x.is_complex() and x.dtype != torch.bool
    return np.asarray(x).dtype.kind in "iu"


def _check_wide_pid(pid) -> None:
    if not (isinstance(pid, (torch.Tensor, np.ndarray)) and _integer_like(pid)):
        raise TypeError("wide_privacy_ids=True needs integers: an integer tensor or array of "
                        "privacy ids")


def _check_string_columns(pid, pk, n_partitions, sparse, pid_range) -> None:
    """The options a StringColumn excludes; host state only."""
    if isinstance(pk, StringColumn):
        if n_partitions is not None:
            raise ValueError("a StringColumn of partition keys gets its dense ids from the "
                             "device dictionary: n_partitions must not be given")
        if sparse:
            raise ValueError("sparse_partition_keys=True needs integer partition keys, not a "
                             "StringColumn (which has a device dictionary of its own)")
    if isinstance(pid, StringColumn) and pid_range is not None:
        raise ValueError("a StringColumn of privacy ids is hashed to wide privacy ids: "
                         "privacy_id_range must not be given")


def _is_int_key(k) -> bool:
    return isinstance(k, (int, np.integer)) and not isinstance(k, bool)


def _encode_keys(values, device, extra=None):
    """Dictionary-encodes arbitrary keys; returns (ids tensor, key table,
    ids of `extra`)."""
    if isinstance(values, torch.Tensor) and _integer_like(values):
        extra_i = None
        if extra is not None:
            extra = list(extra)
            if not all(_is_int_key(k) for k in extra):
                # integer data keys, public partitions with other keys: the
                # general (object) encoding; those partitions come out empty
                return _encode_keys(values.cpu().numpy().astype(object), device, extra)
            extra_i = torch.as_tensor(np.asarray(extra, dtype=np.int64), device=values.device)
        both = values if extra is None else torch.cat([values, extra_i])
        uniq, inv = torch.unique(both, return_inverse=True)
        n = values.numel()
        return (inv[:n].to(torch.int64).to(device), uniq.cpu().numpy(),
                None if extra is None else inv[n:].cpu().numpy())
    arr = np.asarray(values, dtype=object) if not isinstance(values, np.ndarray) else values
    if extra is not None:
        arr = np.concatenate([np.asarray(arr, dtype=object),
                              np.asarray(list(extra), dtype=object)])
    try:
        uniq, inv = np.unique(arr, return_inverse=True)
        table = list(uniq)
    except TypeError:  # unorderable keys: first-seen order
        index = {}
        inv = np.empty(len(arr), dtype=np.int64)
        for i, k in enumerate(arr.tolist()):
            inv[i] = index.setdefault(k, len(index))
        table = list(index)
    n = len(values)
    ids = torch.from_numpy(np.ascontiguousarray(inv[:n].astype(np.int64))).to(device)
    return ids, table, (None if extra is None else inv[n:])


def _public_id_tensor(public_partitions, device) -> Optional[torch.Tensor]:
    """Integer public partitions given as a range, ndarray or tensor, as a
    device int64 tensor (None for other containers, which are listed)."""
    if isinstance(public_partitions, range):
        r = public_partitions
        return torch.arange(r.start, r.stop, r.step, dtype=torch.int64, device=device)
    if isinstance(public_partitions, (torch.Tensor, np.ndarray)) and _integer_like(public_partitions):
        return _to_tensor(public_partitions, device).to(torch.int64).reshape(-1)
    return None


def _sparse_public_keys(public_partitions, device) -> torch.Tensor:
    """The public partitions of a sparse_partition_keys input as a device
    int64 tensor: an integer range, list, array or tensor; else TypeError."""
    t = _public_id_tensor(public_partitions, device)
    if t is None and isinstance(public_partitions, (list, tuple)) and all(
            _is_int_key(k) for k in public_partitions):
        try:
            t = torch.from_numpy(np.asarray(public_partitions, dtype=np.int64)
                                 .reshape(-1)).to(device)
        except OverflowError:
            t = None
    if t is None:
        raise TypeError("sparse_partition_keys=True needs integer public partitions: a range, "
                        "list, array or tensor of int64 keys, the same on every rank")
    return t


def _check_public_range(lo: int, hi: int, P: int) -> None:
    if lo < 0 or hi >= P:
        raise ValueError(
            f"public partition id {lo if lo < 0 else hi} is outside [0, n_partitions={P}): with "
            f"ColumnarData(n_partitions=P) every partition key, public ones included, must be a "
            f"dense id in [0, P)")


def _device_bitmap(ids: torch.Tensor, P: int, device) -> Tuple[torch.Tensor, int]:
    """Bitmap of P bits (bit i of byte i >> 3 = partition i public) built on
    the device, and the number of distinct ids (all must lie in [0, P))."""
    if ids.numel():
        _check_public_range(*_range(ids), P)
    flags = torch.zeros(((P + 7) // 8) * 8, dtype=torch.uint8, device=device)
    flags[ids] = 1
    count = int(flags.sum(dtype=torch.int64).item())
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=device)
    mask = (flags.view(-1, 8) * w).sum(1, dtype=torch.uint8)
    return mask.contiguous(), count


def _range_bitmap(lo: int, hi: int, P: int, device) -> Tuple[torch.Tensor, int]:
    """The _device_bitmap of range(lo, hi) without materialising the ids
    (config 4's public_partitions = range(1e8): 800 MB of ids, a scatter
    and two reductions per release otherwise)."""
    mask = torch.zeros((P + 7) // 8, dtype=torch.uint8, device=device)
    if hi <= lo:
        return mask, 0
    _check_public_range(lo, hi - 1, P)
    b0, b1 = lo >> 3, (hi - 1) >> 3
    head = (0xFF << (lo & 7)) & 0xFF
    tail = 0xFF >> (7 - ((hi - 1) & 7))
    if b0 == b1:
        mask[b0] = head & tail
    else:
        mask[b0] = head
        mask[b0 + 1:b1] = 0xFF
        mask[b1] = tail
    return mask, hi - lo


def _range(t: torch.Tensor):
    if t.numel() == 0:
        return 0, -1
    return int(t.min().item()), int(t.max().item())


def encode(col, extractors, device: torch.device, need_values: bool,
           public_partitions=None, need_pid: bool = True,
           allow_sparse: bool = False, vector_size: Optional[int] = None,
           ctx=None, world_size: int = 1, group=None) -> EncodedInput:
    """`ctx`: the library context of the backend, which a StringColumn needs
    (NotImplementedError without); `world_size`: the backend's, since a string
    `pk` runs in one process only unless ColumnarData(global_string_keys=True)
    asks for the global string dictionary, which is then built here over the
    process group `group` (None: one process).  Every returned column is contiguous (a copy only when the caller's is
    not), int64 / float64, on `device`, and n elements long: the kernels take
    raw pointers.  `vector_size`: None for scalar metrics, whose value column
    is [n] (or [n, 1], flattened; another shape raises ValueError); with
    VECTOR_SUM the [n, vector_size] shape is the caller's to check."""
    pid_range, rec_off = None, 0
    if _is_columnar(col):
        pid = _extract(col, extractors.privacy_id_extractor) if need_pid else None
        pk = _extract(col, extractors.partition_extractor)
        value = _extract(col, extractors.value_extractor) if need_values else None
        hint = col.n_partitions if isinstance(col, ColumnarData) else col.get("n_partitions")
        if isinstance(col, ColumnarData):
            pid_range, rec_off = col.privacy_id_range, int(col.record_id_offset)
    else:
        rows = col if isinstance(col, list) else list(col)
        ex = extractors
        pid = [ex.privacy_id_extractor(r) for r in rows] if need_pid else None
        pk = [ex.partition_extractor(r) for r in rows]
        value = ([ex.value_extractor(r) for r in rows]
                 if need_values and ex.value_extractor is not None else None)
        hint = None
    if pk is None:
        raise ValueError("partition_extractor must be set")
    n = len(pk)
    if need_values and value is None:
        raise ValueError("value_extractor must be set for SUM, MEAN and VARIANCE")
    # the kernels read n elements of every column through a raw pointer
    if need_pid and pid is not None:
        _check_length("pid", pid, n)
    if need_values:
        _check_length("value", value, n)

    # ---- string columns: what they exclude, from host state only (so every
    # rank raises alike, before any device work or collective)
    str_pk = isinstance(pk, StringColumn)
    str_pid = need_pid and isinstance(pid, StringColumn)
    global_str = isinstance(col, ColumnarData) and col.global_string_keys
    if global_str:
        if not str_pk:
            raise ValueError("global_string_keys=True builds a global string dictionary: pk "
                             "must be a StringColumn")
        if not allow_sparse:  # the analysis, histogram and tune entry points
            raise NotImplementedError(
                "global_string_keys=True is supported by DPEngine.aggregate (COUNT, SUM, "
                "PRIVACY_ID_COUNT, MEAN, VARIANCE) and select_partitions only")
    if str_pk or str_pid:
        _check_string_columns(pid if str_pid else None, pk, hint,
                              isinstance(col, ColumnarData) and col.sparse_partition_keys,
                              pid_range)
        if ctx is None:
            raise NotImplementedError("a StringColumn is encoded on the device: this entry "
                                      "point does not pass the library context to the encoder")
    if str_pk and world_size > 1 and not global_str:
        raise NotImplementedError(
            "a StringColumn of partition keys is supported in one process only: a global "
            "string dictionary across ranks is not built.  Encode the partition keys to dense "
            "ids (ColumnarData(n_partitions=P)) or to int64 keys (sparse_partition_keys=True)")
    if isinstance(public_partitions, StringColumn) and not str_pk:
        public_partitions = public_partitions.to_strings()

    # ---- partition keys -> dense ids
    # dense integer keys with a declared P and array-like public partitions:
    # the public bitmap is built on the device (config 4: 1e8 public ids)
    pub_dense = None
    pub_range = None  # a unit-step range: its bitmap is two partial bytes and a fill
    if public_partitions is not None and hint is not None and not str_pk and _integer_like(pk):
        if isinstance(public_partitions, range) and public_partitions.step == 1:
            pub_range = (public_partitions.start, public_partitions.stop)
        else:
            pub_dense = _public_id_tensor(public_partitions, device)
    # ColumnarData(sparse_partition_keys=True): the keys stay as they are and
    # DeviceAggregation builds their dictionary (every rank the same one)
    sparse = isinstance(col, ColumnarData) and col.sparse_partition_keys
    sparse_public = None
    if sparse:
        if not allow_sparse:  # the analysis, histogram and tune entry points
            raise NotImplementedError(
                "sparse_partition_keys=True is supported by DPEngine.aggregate (COUNT, SUM, "
                "PRIVACY_ID_COUNT, MEAN, VARIANCE) and select_partitions only")
        if hint is not None:
            raise ValueError("sparse_partition_keys=True builds the dense partition ids itself: "
                             "n_partitions must not be given")
        if not _integer_like(pk):
            raise TypeError("sparse_partition_keys=True needs an integer tensor or array of "
                            "partition keys")
        if public_partitions is not None:
            sparse_public = _sparse_public_keys(public_partitions, device)
    public_list = (None if public_partitions is None or pub_dense is not None
                   or pub_range is not None or sparse or str_pk else list(public_partitions))
    key_table = None
    pk_ids = None
    public_ids = None
    # rows whose partition keys are numpy scalars keep those objects as the
    # key table: results and the utility analysis' partition sampler then see
    # the user's own keys (repr np.int64(5), as the reference's rows print).
    # Only without an n_partitions hint: with one, the keys are the caller's
    # dense ids, and the public bitmap above (pub_range / pub_dense) was
    # built over those ids, so they must not be re-encoded
    np_row_keys = (hint is None and not sparse and isinstance(pk, list)
                   and any(isinstance(k, np.generic) for k in pk))
    string_dictionary = None
    if global_str:
        # hashed and verified on the device, ids from the hashes, the strings
        # checked and kept by their hashes' owners; none reaches the host here
        string_dictionary = string_columns.encode_global_partition_keys(
            pk, string_columns.public_strings(public_partitions), device, ctx,
            col.max_distinct_partition_keys, group)
        pk_ids, P = string_dictionary.ids, string_dictionary.n_partitions
        if string_dictionary.public_ids is not None:
            public_ids = string_dictionary.public_ids.cpu().numpy()
    elif str_pk:
        # hashed, verified and dictionary-encoded on the device; only the
        # distinct strings reach the host
        pk_ids, key_table, public_ids = string_columns.encode_partition_keys(
            pk, string_columns.public_strings(public_partitions), device, ctx,
            col.max_distinct_partition_keys if isinstance(col, ColumnarData) else None)
        P = max(len(key_table), 1)
    elif _integer_like(pk) and not np_row_keys:
        pk_t = _to_tensor(pk, device).to(torch.int64)
        if sparse:
            pk_ids, P = pk_t, 1  # P: a placeholder until the dictionary is built
        elif hint is not None:
            P = int(hint)
            pk_ids = pk_t
            if public_list is not None:
                public_ids = np.asarray(public_list, dtype=np.int64)
        else:
            lo, hi = _range(pk_t)
            pub_arr = None
            if public_list is not None:
                try:
                    pub_arr = np.asarray(public_list, dtype=np.int64)
                except (TypeError, ValueError, OverflowError):
                    pub_arr = None
                if pub_arr is not None and pub_arr.size:
                    lo, hi = min(lo, int(pub_arr.min())), max(hi, int(pub_arr.max()))
            dense_ok = lo >= 0 and hi + 1 <= max(1 << 20, 4 * max(n, 1)) and (
                public_list is None or pub_arr is not None)
            if dense_ok:
                pk_ids, P = pk_t, max(hi + 1, 1)
                public_ids = pub_arr
            else:
                pk_ids, key_table, public_ids = _encode_keys(pk_t, device, public_list)
                P = max(len(key_table), 1)
    else:
        pk_ids, key_table, public_ids = _encode_keys(pk, device, public_list)
        P = max(len(key_table), 1)

    # ---- privacy ids -> integers spanning <= 2^32 values, with their range
    # when known (else the device reduces it)
    pid_ids = None
    pid_min, pid_count = 0, 0
    pid_unencoded = False
    # ColumnarData(wide_privacy_ids=True): the ids stay as they are and
    # distributed.encode_privacy_ids builds the rank's dictionary once the
    # records are placed
    wide = need_pid and isinstance(col, ColumnarData) and col.wide_privacy_ids
    pid_bad_offsets = None
    if need_pid:
        if pid is None:
            raise ValueError("privacy_id_extractor must be set")
        if str_pid:
            # the column becomes its 64-bit hashes: wide privacy ids from here
            # on.  The invalid-offset count stays on the device until
            # encode_privacy_ids agrees on the errors of every rank
            pid_ids, pid_bad_offsets = string_columns.device_keys(
                *pid.device_columns(device), pid.hash_seed, ctx)
            pid_unencoded = True
            wide = True
        elif wide:
            if pid_range is not None:
                raise ValueError("wide_privacy_ids=True encodes the privacy ids itself: "
                                 "privacy_id_range must not be given")
            _check_wide_pid(pid)
            pid_ids = _to_tensor(pid, device).to(torch.int64)
            pid_unencoded = True
        elif _integer_like(pid):
            pid_t = _to_tensor(pid, device).to(torch.int64)
            pid_unencoded = True
            if pid_range is not None:
                lo, hi = int(pid_range[0]), int(pid_range[1])
                if not 0 < hi - lo <= _PID_SPAN:
                    raise ValueError("privacy_id_range must be (lo, hi) with 0 < hi - lo <= 2^32")
                pid_min, pid_count = lo, hi - lo
            elif hint is None and n > 0:
                lo, hi = _range(pid_t)
                if hi - lo >= _PID_SPAN:
                    pid_t, uniq, _ = _encode_keys(pid_t, device)
                    pid_min, pid_count = 0, max(1, len(uniq))
                    pid_unencoded = False
                else:
                    pid_min, pid_count = lo, hi - lo + 1
            pid_ids = pid_t
        else:
            pid_ids, table, _ = _encode_keys(pid, device)
            pid_min, pid_count = 0, max(1, len(table))

    val = None
    if need_values:
        val = _to_tensor(value, device).to(torch.float64)
        if vector_size is None:
            if val.dim() == 2 and val.shape[1] == 1:
                val = val.reshape(-1)
            elif val.dim() != 1:
                raise ValueError(
                    f"the value column has shape {tuple(val.shape)}: SUM, MEAN, VARIANCE and "
                    f"PERCENTILE need one value per record, shape ({n},) or ({n}, 1)")
        val = val.contiguous()

    enc = EncodedInput(pid=pid_ids, pk=pk_ids.contiguous(), value=val, n=n,
                       n_partitions=int(P), key_table=key_table, pid_min=pid_min,
                       pid_count=pid_count, rec_id_offset=rec_off,
                       partitions_declared=(hint is not None and key_table is None) or global_str,
                       pid_unencoded=pid_unencoded,
                       pid_range_declared=pid_unencoded and pid_range is not None,
                       pk_sparse=bool(sparse), public_keys=sparse_public, pid_wide=bool(wide),
                       max_distinct_pids=(col.max_distinct_privacy_ids
                                          if wide and isinstance(col, ColumnarData) else None),
                       pid_bad_offsets=pid_bad_offsets, string_dictionary=string_dictionary)
    if pub_range is not None:
        enc.public_mask, enc.public_count = _range_bitmap(*pub_range, int(P), device)
    elif pub_dense is not None:
        enc.public_mask, enc.public_count = _device_bitmap(pub_dense, int(P), device)
    elif public_ids is not None:
        mask = np.zeros((P + 7) // 8, dtype=np.uint8)
        ids = np.unique(np.asarray(public_ids, dtype=np.int64))
        if ids.size and key_table is None:
            _check_public_range(int(ids[0]), int(ids[-1]), P)
        np.bitwise_or.at(mask, ids >> 3, (1 << (ids & 7)).astype(np.uint8))
        enc.public_mask = torch.from_numpy(mask).to(device)
        enc.public_count = int(ids.size)
    if enc.pid is not None:
        enc.pid = enc.pid.contiguous()
    return enc


def decode_keys(ids: np.ndarray, key_table) -> list:
    """Dense ids -> the user's keys, as Python objects: a numpy key table
    (integer tensor / array columns) yields Python scalars, so a key prints
    and hashes as the reference's row keys do (e.g. repr 5, not
    np.int64(5), which the utility analysis' partition sampler hashes)."""
    if key_table is None:
        return ids.tolist()
    if isinstance(key_table, np.ndarray):
        return key_table[ids].tolist()
    return [key_table[i] for i in ids.tolist()]
