"""Lazy device execution of one DPEngine.aggregate / select_partitions call.

The reference returns a lazy collection whose generators run when the user
iterates it, after `BudgetAccountant.compute_budgets()` (SURVEY.md 3.4;
pinned by the reference's tests/pipeline_backend_test.py:564-591).  This
object keeps that contract: nothing touches the GPU until the first
`__iter__` / `materialize()`, and budgets are read at that moment.

Device pipeline per call (include/dpg.h):
  dpg_bound_aggregate -> [multi-GPU: reduce-scatter of the dense partials,
  or a fixed-block all-to-all of the occupied ones, with every rank's error
  flag: distributed.exchange_partials] -> dpg_select_and_noise ->
  dpg_compact_kept_async.  A plan with percentiles adds dpg_bound_records and
  dpg_quantile_keys behind the bounding and dpg_quantiles behind the
  selection, whose columns join the noise kernel's.  A plan with VECTOR_SUM
  adds dpg_bound_records, dpg_vector_index and dpg_vector_sums behind the
  bounding and dpg_vector_clip_noise behind the selection; its D columns come
  last.  With several ranks the sorted tree keys, or the occupied partitions'
summed rows, follow the partials to the partitions' owners
(distributed.exchange_owner_keys: dpg_owner_split_keys, one more host
synchronisation) and are merged there by dpg_sort_pairs_u64, or by
dpg_vector_index and dpg_vector_sums.  The kept count reaches the host when the result's
  ids or values are first read (the one host synchronisation after the
  bounding), so a caller can enqueue the next release first.
"""
import ctypes
import os
import warnings
from typing import Optional, Sequence

import numpy as np
import torch

from pipelinedp_amd import _native
from pipelinedp_amd import columnar
from pipelinedp_amd import combiners
from pipelinedp_amd import distributed
from pipelinedp_amd import partition_selection
from pipelinedp_amd import string_columns


# experiments: DPG_SYNC_COMPACT=1 synchronises at the compaction, as before
# round 5 (same-box A/B of the asynchronous result)
_SYNC_COMPACT = os.environ.get("DPG_SYNC_COMPACT", "0") == "1"


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# Results dropped before their device info word was read: their
# bounding error bits are checked when the release has finished, at the
# latest by the next release on any backend, and reported as a warning.
_DROPPED = []


def check_dropped(block: bool = False) -> None:
    """Warns about dropped, never-read results whose bounding latched an
    internal error; block=True waits for the unfinished ones."""
    keep = []
    for info, ev in _DROPPED:
        if ev is not None and not block and not ev.query():
            keep.append((info, ev))
            continue
        if ev is not None:
            ev.synchronize()
        if int(info[1].item()) & 2:
            warnings.warn("a DeviceResult dropped without being read had an internal bounding "
                          "error (hash-table overflow); its release was invalid", RuntimeWarning)
    _DROPPED[:] = keep


class DeviceResult:
    """Materialised result: kept partition ids (int64 [K], global dense ids;
    with ColumnarData(sparse_partition_keys=True) the caller's int64 keys)
    and their metric columns (float64 [K, len(fields)]), on the device; with
    VECTOR_SUM the last field `vector_sum` takes the last vector_size columns
    ([K, n_scalar + D]).  `keys()` maps ids back to the user's partition keys.

    Built from the compaction's full-size outputs and its device info word
    (kept count, bounding error bits): the count is read -- and an internal
    bounding error raised -- when `partition_ids` or `values` is first used."""

    def __init__(self, partition_ids: torch.Tensor, values: torch.Tensor, fields: tuple,
                 key_table: Optional[Sequence], stage_ms: Optional[dict] = None,
                 pending: Optional[tuple] = None, key_map: Optional[torch.Tensor] = None,
                 string_dictionary=None, strings: Optional[list] = None):
        self._ids, self._vals = partition_ids, values
        # global_string_keys: the kept local ids also index the owner's string
        # table, from which keys() packs and decodes the kept strings -- or
        # `strings` holds them already (gathered from every rank)
        self._string_dictionary = string_dictionary
        self._strings = strings
        self._local_ids = None
        # sparse partition keys: the kept local ids index this int64 tensor of
        # the caller's keys (the rank's owned keys) instead of being re-based
        self._key_map = key_map
        self.fields = fields
        self.key_table = key_table
        self.stage_ms = stage_ms if stage_ms is not None else {}
        # (info int64[2] on the device, outputs per row, id stride, id offset
        # [, event recorded behind the compaction on the release's stream])
        self._pending = pending

    def _resolve(self):
        if self._pending is None:
            return
        info, n_out, stride, offset = self._pending[:4]
        if len(self._pending) > 4 and self._pending[4] is not None:
            # the release ran on the stream current at materialize(); the
            # reader's current stream may be another one
            self._pending[4].synchronize()
        k, err = (int(x) for x in info.tolist())
        if err & 2:
            self._pending = None  # reported here, not again when dropped
            raise _native.NativeError(
                "dpg_compact_kept failed (HIP error): internal hash-table error in bounding")
        ids = self._ids[:k]
        if self._string_dictionary is not None:
            self._local_ids = ids.clone()
        if self._key_map is not None:
            ids = self._key_map[ids]
        elif stride != 1 or offset:  # several ranks: this rank's slice
            ids = ids * stride + offset
        vals = (self._vals[:k * n_out].view(k, n_out) if n_out
                else torch.empty((k, 0), dtype=torch.float64, device=self._vals.device))
        # a small kept set does not pin the partition-sized compaction
        # buffers: compact copies
        if 2 * k < self._ids.numel():
            ids = ids.clone() if ids.data_ptr() == self._ids.data_ptr() else ids
            vals = vals.clone()
        self._ids, self._vals = ids, vals
        self._pending = None

    def __del__(self):
        p = getattr(self, "_pending", None)
        if p is not None:
            _DROPPED.append((p[0], p[4] if len(p) > 4 else None))

    @property
    def partition_ids(self) -> torch.Tensor:
        self._resolve()
        return self._ids

    @property
    def values(self) -> torch.Tensor:
        self._resolve()
        return self._vals

    def packed_strings(self):
        """global_string_keys: (offsets int64[K + 1], bytes uint8) of this
        rank's kept partitions' strings, packed on the device from the owner's
        string table (dpg_string_pack)."""
        self._resolve()
        return self._string_dictionary.packed(self._local_ids)

    def keys(self) -> list:
        if self._strings is None and self._string_dictionary is not None:
            # only the kept partitions' strings are ever decoded
            self._strings = string_columns.decode_packed(*self.packed_strings(),
                                                         self._string_dictionary.encoding)
        if self._strings is not None:
            return list(self._strings)
        return columnar.decode_keys(self.partition_ids.cpu().numpy(), self.key_table)


class DeviceAggregation:
    """Lazy collection of (partition_key, MetricsTuple) -- or of partition
    keys for select_partitions."""

    def __init__(self, backend, col, extractors, plan: Optional[combiners.CompoundPlan],
                 public_partitions=None, selection_spec=None, strategy=None,
                 max_partitions_contributed: int = 1, pre_threshold=None,
                 max_rows_per_privacy_id: int = 1, drop_non_public: bool = True,
                 bounds_already_enforced: bool = False, keys_only: bool = False):
        self.backend = backend
        self.col = col
        self.extractors = extractors
        self.plan = plan
        self.public_partitions = public_partitions
        self.selection_spec = selection_spec
        self.strategy = strategy
        self.max_partitions_contributed = max_partitions_contributed
        self.pre_threshold = pre_threshold
        self.max_rows = max_rows_per_privacy_id
        self.drop_non_public = drop_non_public
        self.bounds_already_enforced = bounds_already_enforced
        self.keys_only = keys_only
        self._result: Optional[DeviceResult] = None
        self.last_partials = None
        self.noise_enabled = True
        # Per-release nonce of every keyed random stream (include/dpg.h
        # dpg_stream_seed).  None: drawn from os.urandom when the release is
        # materialised, so two releases on one backend draw independent
        # sampling, selection and noise, like the reference's fresh PyDP /
        # numpy randomness per call (dp_computations.py:131-133, 151-152;
        # pipeline_backend.py:540-544).  Tests inject it to reproduce a
        # release; multi-GPU releases broadcast rank 0's.
        self.nonce: Optional[int] = None
        self.last_bound_fields: Optional[dict] = None
        self.last_exchange: Optional[dict] = None
        self.last_select_fields: Optional[dict] = None
        # sparse_partition_keys: the distributed.KeyDictionary of the release
        self.last_key_dictionary = None
        # global_string_keys: the distributed.StringDictionary of the release
        # (the records' ids, P, and this rank's slice of the string table)
        self.last_string_dictionary = None

    # ------------------------------------------------------------ public
    def __iter__(self):
        res = self.materialize()
        keys = res.keys()
        if self.keys_only:
            return iter(keys)
        vals = res.values.cpu().numpy()
        T = self.plan.MetricsTuple
        D = self.plan.vector_size
        if D is None:
            return iter([(k, T(*map(float, row))) for k, row in zip(keys, vals)])
        # the vector's D columns are the last ones; its field is the last one
        ns = vals.shape[1] - D
        return iter([(k, T(*map(float, row[:ns]), row[ns:].copy()))
                     for k, row in zip(keys, vals)])

    def materialize(self, gather: bool = True) -> DeviceResult:
        if self._result is None:
            self._result = self._run(gather)
        return self._result

    # ------------------------------------------------------------ device
    def _bound_fields(self, P: int) -> dict:
        if self.plan is not None:
            f = self.plan.bound_fields(P)
        else:  # select_partitions: cross-partition bounding, keys only
            f = dict(mode=combiners.MODE_CROSS, sum_mode=combiners.SUM_NONE, metric_mask=0,
                     max_partitions_contributed=self.max_partitions_contributed,
                     max_contributions_per_partition=1, max_contributions=0,
                     min_value=0.0, max_value=0.0, min_sum_per_partition=0.0,
                     max_sum_per_partition=0.0, n_partitions=P)
        if self.bounds_already_enforced:
            # every row is its own privacy unit: bounding never samples
            f.update(mode=combiners.MODE_CROSS_AND_PER if f["mode"] != combiners.MODE_CROSS
                     else combiners.MODE_CROSS,
                     max_partitions_contributed=max(1, f["max_partitions_contributed"]),
                     max_contributions_per_partition=max(1, f["max_contributions_per_partition"]))
            if f["mode"] == combiners.MODE_PER_PID:
                f["mode"] = combiners.MODE_CROSS_AND_PER
        return f

    def _select_fields(self, pk_offset: int, public_mask_local, pk_stride: int = 1) -> dict:
        nonce = self.nonce or 0
        if self.public_partitions is not None:
            return dict(strategy=0, table_len=0, keep_table=None, threshold=0.0,
                        noise_scale=0.0, pre_threshold=0, max_rows_per_privacy_id=1,
                        pk_offset=pk_offset, pk_stride=pk_stride, public_mask=public_mask_local,
                        nonce=nonce)
        spec = self.selection_spec
        sp = partition_selection.create_partition_selection_strategy(
            self.strategy, spec.eps, spec.delta, self.max_partitions_contributed,
            self.pre_threshold)
        self._selection_plan = sp
        f = dict(strategy=sp.native_strategy, table_len=0, keep_table=None,
                 threshold=sp.threshold, noise_scale=sp.noise_scale,
                 pre_threshold=int(self.pre_threshold or 0),
                 max_rows_per_privacy_id=int(self.max_rows), pk_offset=pk_offset,
                 pk_stride=pk_stride, public_mask=None, nonce=nonce)
        if sp.table is not None:
            self._table = np.ascontiguousarray(np.asarray(sp.table, dtype=np.float64))
            f["table_len"] = len(self._table)
            f["keep_table"] = self._table.ctypes.data
        return f

    def _release_header(self, nnz_bound: int):
        """The release nonce (rank 0's) and, with several ranks, the
        occupancy bound maximised over ranks: one collective, before any
        device work of the release."""
        if self.nonce is None:
            self.nonce = int.from_bytes(os.urandom(8), "little")
        if self.backend.world_size > 1:
            self.nonce, nnz_bound = distributed.release_header(
                self.nonce, nnz_bound, self.backend.process_group, self.backend.device)
        return self.nonce, nnz_bound

    def _place_records(self, enc) -> None:
        """ColumnarData(sharding=...) with several ranks: 'verify' checks that
        this rank owns every privacy id it holds (one kernel, one all_reduce;
        every rank raises when any rank fails), 'shuffle' sends every record
        to its owner (distributed.shuffle_records) and bounds what arrives."""
        mode = self.col.sharding if isinstance(self.col, columnar.ColumnarData) else "trusted"
        if self.bounds_already_enforced:
            return
        distributed.place_records(enc, self.backend, mode)

    def _encode_sparse_keys(self, enc) -> None:
        """ColumnarData(sparse_partition_keys=True): replaces the caller's
        int64 partition keys in `enc` by global dense ids, the same on every
        rank (distributed.build_key_dictionary: the hash-dictionary kernels,
        with several ranks four collectives), before the records are placed.
        The public bitmap is built over the public keys' ids; the result maps
        the kept local ids back through this rank's owned keys."""
        backend = self.backend
        dev = backend.device
        group = backend.process_group if backend.world_size > 1 else None
        with torch.cuda.device(dev):
            sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            kd = distributed.build_key_dictionary(
                enc.pk, enc.public_keys, group, backend.ctx, sptr,
                max_distinct=self.col.max_distinct_partition_keys)
            enc.pk = kd.ids
            enc.n_partitions = kd.n_partitions
            enc.partitions_declared = True
            enc.pk_sparse = False
            if kd.public_ids is not None:
                enc.public_mask, enc.public_count = columnar._device_bitmap(
                    kd.public_ids, kd.n_partitions, dev)
        self.last_key_dictionary = kd

    def _own_quantile_keys(self, qkeys, n_qkeys, local_P: int, sptr):
        """Several ranks: this rank's sorted tree keys pk << 16 | leaf go to
        their partitions' owners (distributed.exchange_owner_keys: one split,
        one host synchronisation, two collectives) and come back as
        pk_local << 16 | leaf, one sorted run per source rank; a keys-only
        sort merges the runs.  Returns the owned keys and their count on the
        device, as dpg_quantiles reads them."""
        backend = self.backend
        dev = backend.device
        got, _, total = distributed.exchange_owner_keys(
            qkeys, n_qkeys, 16, backend.process_group, backend.ctx, sptr)
        keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        backend.ctx.sort_pairs_u64(got.data_ptr(), None, total, 0,
                                   16 + max(local_P - 1, 0).bit_length(), keys.data_ptr(), None,
                                   sptr)
        return keys, torch.tensor([total], dtype=torch.int64, device=dev)

    def _own_vector_sums(self, rows, vsums, P: int, local_P: int, nnz_bound: int, sptr):
        """Several ranks: the rows of this rank's occupied partitions (rows >
        0, ascending: one fixed-size nonzero, the count stays on the device)
        go to the partitions' owners with their partition id as key.  The
        owner indexes the (pk_local, row) pairs it received -- source-rank
        order, so a partition's rows are ascending by source rank -- and
        adds them with dpg_vector_sums.  Returns the merged [local_P, D] sums
        of the owned slice."""
        backend = self.backend
        ctx, dev = backend.ctx, backend.device
        D = vsums.shape[1]
        occ = rows > 0
        n_occ = torch.count_nonzero(occ).reshape(1)
        K = max(1, min(P, int(nnz_bound)))
        idx = torch.nonzero_static(occ, size=K, fill_value=0).view(-1)
        got, got_rows, total = distributed.exchange_owner_keys(
            idx, n_occ, 0, backend.process_group, ctx, sptr, payload=vsums.index_select(0, idx))
        merged = torch.empty((local_P, D), dtype=torch.float64, device=dev)
        if local_P == 0:
            return merged
        keep_all = torch.ones(max(total, 1), dtype=torch.uint8, device=dev)
        vkeys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        n_vkeys = torch.empty(1, dtype=torch.int64, device=dev)
        ctx.vector_index(_ptr(got), keep_all.data_ptr(), total, local_P, vkeys.data_ptr(),
                         n_vkeys.data_ptr(), sptr)
        ctx.vector_sums(vkeys.data_ptr(), n_vkeys.data_ptr(), _ptr(got_rows), total, D, local_P,
                        merged.data_ptr(), sptr)
        return merged

    def _run(self, gather: bool) -> DeviceResult:
        if _DROPPED:
            check_dropped()
        backend = self.backend
        ctx = backend.ctx
        dev = backend.device
        need_values = self.plan is not None and self.plan.needs_values()
        sparse = isinstance(self.col, columnar.ColumnarData) and self.col.sparse_partition_keys
        if sparse and self.plan is not None and (self.plan.percentiles
                                                  or self.plan.vector_size is not None):
            # host state only: every rank raises alike, before any collective
            raise NotImplementedError(
                "sparse_partition_keys=True supports COUNT, SUM, PRIVACY_ID_COUNT, MEAN and "
                "VARIANCE; PERCENTILE and VECTOR_SUM need dense partition ids "
                "(ColumnarData(n_partitions=P))")
        strkeys = isinstance(self.col, columnar.ColumnarData) and self.col.global_string_keys
        if strkeys and self.plan is not None and (self.plan.percentiles
                                                   or self.plan.vector_size is not None):
            # host state only: every rank raises alike, before any collective
            raise NotImplementedError(
                "global_string_keys=True supports COUNT, SUM, PRIVACY_ID_COUNT, MEAN and "
                "VARIANCE; PERCENTILE and VECTOR_SUM need the one-process string route or dense "
                "partition ids (ColumnarData(n_partitions=P))")
        enc = columnar.encode(self.col, self.extractors, dev, need_values,
                              self.public_partitions,
                              need_pid=not self.bounds_already_enforced, allow_sparse=True,
                              vector_size=self.plan.vector_size if self.plan is not None else None,
                              ctx=ctx, world_size=backend.world_size,
                              group=backend.process_group if backend.world_size > 1 else None)
        self.last_string_dictionary = enc.string_dictionary
        if enc.pk_sparse:
            self._encode_sparse_keys(enc)
        if self.bounds_already_enforced:
            enc.pid = torch.arange(enc.n, dtype=torch.int64, device=dev)
            enc.pid_min, enc.pid_count = 0, max(1, enc.n)
        # noise / selection parameters are resolved now (after compute_budgets)
        noise = (self.plan.noise_fields(self.noise_enabled) if self.plan is not None else
                 dict(noise_kind=0, family=0, slot_mask=0, n_outputs=0, out_src=[0] * 8,
                      scale=[0.0] * 4, mid=0.0, mean_const=0, msq_const=0,
                      mean_const_value=0.0, msq_const_value=0.0))
        P = enc.n_partitions
        percentiles = self.plan is not None and bool(self.plan.percentiles)
        if backend.world_size > 1 and not enc.partitions_declared:
            # every rank must use the same dense partition ids and P, or the
            # exchange sums partials of different keys (or hangs)
            raise ValueError(distributed.DENSE_IDS_ERROR)
        vector = self.plan.vector_size if self.plan is not None else None
        if vector is not None:
            # the reference's error class for a vector of another size
            if enc.value.dim() != 2 or tuple(enc.value.shape) != (enc.n, vector):
                raise TypeError(
                    f"Shape mismatch: the value column has shape {tuple(enc.value.shape)}, "
                    f"VECTOR_SUM with vector_size={vector} needs ({enc.n}, {vector})")
            enc.value = enc.value.to(torch.float64).contiguous()
        self._place_records(enc)
        # wide_privacy_ids: this rank's records get their dense privacy ids
        distributed.encode_privacy_ids(enc, backend)
        bfields = self._bound_fields(P)
        l0 = (bfields["max_contributions"] if bfields["mode"] == combiners.MODE_PER_PID
              else bfields["max_partitions_contributed"])
        nonce, nnz_bound = self._release_header(distributed.occupancy_bound(
            P, enc.n, enc.pid_count, int(l0)))
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            sptr = ctypes.c_void_p(stream.cuda_stream)
            f64 = dict(dtype=torch.float64, device=dev)
            rows = torch.empty(P, dtype=torch.int64, device=dev)
            count = torch.empty(P, dtype=torch.int64, device=dev)
            mask = self.plan.mask if self.plan is not None else 0
            sum_ = torch.empty(P, **f64) if mask & combiners.M_SUM else None
            var = mask & (combiners.M_MEAN | combiners.M_VARIANCE)
            nsum = torch.empty(P, **f64) if var else None
            nsq = torch.empty(P, **f64) if var else None
            bound = _native.fill(_native.BoundParams, bfields)
            bound.pid_min, bound.pid_count = enc.pid_min, enc.pid_count
            bound.rec_id_offset = enc.rec_id_offset
            bound.nonce = nonce
            self.last_bound_fields = dict(bfields, pid_min=enc.pid_min, pid_count=enc.pid_count,
                                          rec_id_offset=enc.rec_id_offset, nonce=nonce)
            # _drop_partitions (dp_engine.py:280-286) in the level-1 pass; a
            # public set that covers every partition id drops nothing, so
            # the per-record bitmap lookups are skipped
            if (enc.public_mask is not None and self.drop_non_public
                    and enc.public_count < enc.n_partitions):
                bound.public_mask = enc.public_mask.data_ptr()
            partials = _native.Partials(P, rows.data_ptr(), count.data_ptr(),
                                        sum_.data_ptr() if sum_ is not None else None,
                                        nsum.data_ptr() if nsum is not None else None,
                                        nsq.data_ptr() if nsq is not None else None)
            # a vector column is [n, D]: the bounding has no value lanes then
            # (VECTOR_SUM excludes SUM / MEAN / VARIANCE) and must not see it
            ctx.bound_aggregate(_ptr(enc.pid), _ptr(enc.pk),
                                _ptr(enc.value) if need_values and vector is None else None,
                                enc.n, bound, partials, sptr)
            if vector is not None:
                # the same kept set, record by record, indexed by partition,
                # and the unclipped sums of its rows
                vfields = self.plan.vector_fields(self.noise_enabled)
                rec_keep = torch.empty(max(enc.n, 1), dtype=torch.uint8, device=dev)
                ctx.bound_records(_ptr(enc.pid), _ptr(enc.pk), enc.n, bound,
                                  rec_keep.data_ptr(), sptr)
                vkeys = torch.empty(max(enc.n, 1), dtype=torch.int64, device=dev)
                n_vkeys = torch.empty(1, dtype=torch.int64, device=dev)
                ctx.vector_index(_ptr(enc.pk), rec_keep.data_ptr(), enc.n, P,
                                 vkeys.data_ptr(), n_vkeys.data_ptr(), sptr)
                vsums = torch.empty((P, vector), **f64)
                ctx.vector_sums(vkeys.data_ptr(), n_vkeys.data_ptr(), _ptr(enc.value), enc.n,
                                vector, P, vsums.data_ptr(), sptr)
                self.last_record_keep = rec_keep[:enc.n]
                self.last_vector_sums = vsums
            if percentiles:
                # the same kept set, record by record, and its sorted tree keys
                qfields = self.plan.quantile_fields(self.noise_enabled)
                qp = _native.fill(_native.QuantileParams,
                                  dict(qfields, pk_offset=0, pk_stride=1, nonce=nonce))
                rec_keep = torch.empty(max(enc.n, 1), dtype=torch.uint8, device=dev)
                ctx.bound_records(_ptr(enc.pid), _ptr(enc.pk), enc.n, bound,
                                  rec_keep.data_ptr(), sptr)
                qkeys = torch.empty(max(enc.n, 1), dtype=torch.int64, device=dev)
                n_qkeys = torch.empty(1, dtype=torch.int64, device=dev)
                ctx.quantile_keys(_ptr(enc.pk), _ptr(enc.value), rec_keep.data_ptr(), enc.n, P,
                                  qp, qkeys.data_ptr(), n_qkeys.data_ptr(), sptr)
                self.last_record_keep = rec_keep[:enc.n]
            stage_ms = {}
            tensors = dict(rows=rows, count=count, sum=sum_, nsum=nsum, nsq=nsq)
            self.last_partials = tensors
            pk_offset, pk_stride, local_P = 0, 1, P
            public_mask_local = enc.public_mask
            self.last_exchange = None
            if backend.world_size > 1:
                err = torch.empty(1, **f64)
                ctx.export_error(err.data_ptr(), sptr)
                tensors, (pk_offset, pk_stride, local_P), self.last_exchange, flags = \
                    distributed.exchange_partials(tensors, P, backend.process_group,
                                                  backend.exchange, nnz_bound, err, ctx, sptr)
                # any rank's bounding error fails this rank's compaction
                flags = flags.to(dev).contiguous()
                ctx.import_error(flags.data_ptr(), flags.numel(), sptr)
                if public_mask_local is not None:
                    public_mask_local = distributed.slice_bitmap(
                        enc.public_mask, pk_offset, pk_stride, local_P)
                if percentiles:
                    qkeys, n_qkeys = self._own_quantile_keys(qkeys, n_qkeys, local_P, sptr)
                    qp = _native.fill(_native.QuantileParams,
                                      dict(qfields, pk_offset=pk_offset, pk_stride=pk_stride,
                                           nonce=nonce))
                if vector is not None:
                    vsums = self._own_vector_sums(rows, vsums, P, local_P, nnz_bound, sptr)
                    self.last_vector_sums = vsums
            # this rank's merged partitions pk_offset + i * pk_stride, i < local_P
            self.last_slice = (tensors, pk_offset, pk_stride, local_P)
            lp = _native.Partials(local_P, tensors["rows"].data_ptr(),
                                  tensors["count"].data_ptr(),
                                  *(tensors[k].data_ptr() if tensors[k] is not None else None
                                    for k in ("sum", "nsum", "nsq")))
            sfields = self._select_fields(
                pk_offset, public_mask_local.data_ptr() if public_mask_local is not None else None,
                pk_stride)
            self.last_select_fields = sfields
            sel = _native.fill(_native.SelectParams, sfields)
            nz = _native.fill(_native.NoiseParams, noise)
            n_out = noise["n_outputs"]
            keep = torch.empty(local_P, dtype=torch.uint8, device=dev)
            out = torch.empty(max(local_P * n_out, 1), **f64)
            ctx.select_and_noise(lp, sel, nz, keep.data_ptr(), out.data_ptr(), sptr)
            if percentiles:
                Q = qfields["n_quantiles"]
                qout = torch.zeros((local_P, Q), **f64)
                ctx.quantiles(qkeys.data_ptr(), n_qkeys.data_ptr(), local_P, qp, keep.data_ptr(),
                              qout.data_ptr(), sptr)
                out = (torch.cat([out[:local_P * n_out].view(local_P, n_out), qout], dim=1)
                       .contiguous().view(-1) if n_out else qout.view(-1))
                n_out += Q
            if vector is not None:
                vp = _native.fill(_native.VectorParams,
                                  dict(vfields, pk_offset=pk_offset, pk_stride=pk_stride,
                                       nonce=nonce))
                vout = torch.zeros((local_P, vector), **f64)
                ctx.vector_clip_noise(vsums.data_ptr(), local_P, vp, keep.data_ptr(),
                                      vout.data_ptr(), sptr)
                out = (torch.cat([out[:local_P * n_out].view(local_P, n_out), vout], dim=1)
                       .contiguous().view(-1) if n_out else vout.view(-1))
                n_out += vector
            ids = torch.empty(local_P, dtype=torch.int64, device=dev)
            kept_out = torch.empty(max(local_P * n_out, 1), **f64)
            fields = self.plan.fields if self.plan is not None else ()
            if _SYNC_COMPACT:  # A/B switch: the synchronising compaction
                k = ctx.compact(keep.data_ptr(), out.data_ptr(), local_P, n_out,
                                ids.data_ptr(), kept_out.data_ptr(), sptr)
                info = torch.tensor([k, 0], dtype=torch.int64, device=dev)
            else:
                info = torch.empty(2, dtype=torch.int64, device=dev)
                ctx.compact_async(keep.data_ptr(), out.data_ptr(), local_P, n_out,
                                  ids.data_ptr(), kept_out.data_ptr(), info.data_ptr(), sptr)
            done = torch.cuda.Event()
            done.record(stream)
            # sparse partition keys: the owner turns its kept local ids into the
            # caller's keys (its slice of the dictionary; no global key table)
            # global string keys: the same with the owned hashes, and the owned
            # string table behind them for keys()
            sd = self.last_string_dictionary
            kd = self.last_key_dictionary if sparse else sd
            key_map = None
            if kd is not None:
                # local_P entries: the ids past this owner's keys are holes,
                # never public and never occupied, so never kept
                key_map = torch.zeros(local_P, dtype=torch.int64, device=dev)
                key_map[:kd.owned_keys.numel()] = kd.owned_keys
            res = DeviceResult(ids, kept_out, fields, enc.key_table, stage_ms,
                               pending=(info, n_out, pk_stride, pk_offset, done),
                               key_map=key_map, string_dictionary=sd)
            if backend.world_size > 1 and gather:
                ids, vals, sizes = distributed.all_gather_results(
                    res.partition_ids, res.values, backend.process_group,
                    exact_ids=kd is not None, return_sizes=True)
                strings = None
                if sd is not None:
                    # the kept strings follow in the same rank order: two more
                    # all_gathers, lengths and bytes
                    strings = distributed.all_gather_strings(
                        *res.packed_strings(), sizes, backend.process_group, sd.encoding)
                res = DeviceResult(ids, vals, fields, enc.key_table, stage_ms, strings=strings)
        return res
