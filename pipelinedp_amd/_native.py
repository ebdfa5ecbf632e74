"""ctypes binding of libdpg.so (include/dpg.h).

The library is built in-tree by __graft_entry__.build() into
pipelinedp_amd/lib/libdpg.so.  There is no CPU fallback: if the library or a
GPU is missing, every device entry point raises.
"""
import ctypes
import os
import threading

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libdpg.so")

DPG_OK = 0
ERRORS = {1: "invalid argument", 2: "key out of range", 3: "HIP error",
          4: "out of device memory", 5: "unsupported"}

EXPORTED = ("dpg_ctx_create", "dpg_ctx_destroy", "dpg_last_error", "dpg_set_seed",
            "dpg_set_tuning",
            "dpg_bound_aggregate", "dpg_select_and_noise", "dpg_compact_kept",
            "dpg_compact_kept_async", "dpg_last_stage_times", "dpg_stream_seed",
            "dpg_preaggregate",
            "dpg_utility_analysis", "dpg_dataset_histograms",
            "dpg_hist_pairs", "dpg_hist_partitions", "dpg_hist_sums",
            "dpg_comm_unique_id", "dpg_ctx_create_comm", "dpg_reduce_scatter_partials",
            "dpg_pack_partials", "dpg_unpack_partials", "dpg_export_error",
            "dpg_import_error", "dpg_shard_records", "dpg_check_shard",
            "dpg_owner_split_keys", "dpg_owner_split_pairs", "dpg_merge_pair_runs",
            "dpg_sort_pairs_u64", "dpg_bound_records", "dpg_quantile_keys", "dpg_quantiles",
            "dpg_vector_index", "dpg_vector_sums", "dpg_vector_clip_noise",
            "dpg_sample_partitions", "dpg_partition_summary",
            "dpg_keydict_insert", "dpg_keydict_keys", "dpg_keydict_assign",
            "dpg_keydict_lookup", "dpg_keydict_insert_slots", "dpg_keydict_gather_ids",
            "dpg_shard_records_wide", "dpg_check_shard_wide",
            "dpg_string_hash", "dpg_keydict_representatives", "dpg_string_verify",
            "dpg_string_lengths", "dpg_string_pack", "dpg_string_verify_runs")

KEYDICT_EMPTY = 1 << 63  # DPG_KEYDICT_EMPTY: the bit pattern of INT64_MIN, the reserved key
KEYDICT_NO_SLOT = 0xFFFFFFFF  # dpg_keydict_insert_slots: a reserved or lost record

COMM_ID_BYTES = 128  # DPG_COMM_ID_BYTES

SHARD_MAX_RANKS = 64  # DPG_SHARD_MAX_RANKS
SHARD_TILE = 2048  # DPG_SHARD_TILE (csrc/dpg_shard.h): records per workgroup of the split

SLOT_QNODE0 = 16  # DPG_SLOT_QNODE0: noise slot of quantile-tree node 0
QUANTILE_MAX = 16  # quantiles per dpg_quantiles call

SLOT_VEC0 = 1 << 20  # DPG_SLOT_VEC0: noise slot of vector coordinate 0
VECTOR_MAX_SIZE = 4096  # DPG_VECTOR_MAX_SIZE
VSUM_CHUNK = 512  # DPG_VSUM_CHUNK: sorted rows summed by one wave
NORM_LINF, NORM_L1, NORM_L2 = 0, 1, 2  # DPG_NORM_*

HIST_INT_BINS = 16300  # DPG_HIST_INT_BINS
HIST_SUM_BINS = 10000  # DPG_HIST_SUM_BINS


class BoundParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("sum_mode", ctypes.c_int32),
                ("metric_mask", ctypes.c_uint32), ("reserved0", ctypes.c_int32),
                ("max_partitions_contributed", ctypes.c_int64),
                ("max_contributions_per_partition", ctypes.c_int64),
                ("max_contributions", ctypes.c_int64),
                ("min_value", ctypes.c_double), ("max_value", ctypes.c_double),
                ("min_sum_per_partition", ctypes.c_double),
                ("max_sum_per_partition", ctypes.c_double),
                ("n_partitions", ctypes.c_int64), ("public_mask", ctypes.c_void_p),
                ("pid_min", ctypes.c_int64), ("pid_count", ctypes.c_int64),
                ("rec_id_offset", ctypes.c_int64), ("nonce", ctypes.c_uint64)]


class Partials(ctypes.Structure):
    _fields_ = [("n_partitions", ctypes.c_int64), ("rows", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("sum", ctypes.c_void_p),
                ("nsum", ctypes.c_void_p), ("nsq", ctypes.c_void_p)]


class SelectParams(ctypes.Structure):
    _fields_ = [("strategy", ctypes.c_int32), ("table_len", ctypes.c_int32),
                ("keep_table", ctypes.c_void_p), ("threshold", ctypes.c_double),
                ("noise_scale", ctypes.c_double), ("pre_threshold", ctypes.c_int64),
                ("max_rows_per_privacy_id", ctypes.c_int64),
                ("pk_offset", ctypes.c_int64), ("public_mask", ctypes.c_void_p),
                ("nonce", ctypes.c_uint64), ("pk_stride", ctypes.c_int64)]


class NoiseParams(ctypes.Structure):
    _fields_ = [("noise_kind", ctypes.c_int32), ("family", ctypes.c_int32),
                ("slot_mask", ctypes.c_uint32), ("n_outputs", ctypes.c_int32),
                ("out_src", ctypes.c_int32 * 8), ("scale", ctypes.c_double * 4),
                ("mid", ctypes.c_double), ("mean_const", ctypes.c_int32),
                ("msq_const", ctypes.c_int32), ("mean_const_value", ctypes.c_double),
                ("msq_const_value", ctypes.c_double)]


class QuantileParams(ctypes.Structure):
    """dpg_quantile_params: the tree's range, node noise and quantiles."""
    _fields_ = [("lo", ctypes.c_double), ("hi", ctypes.c_double),
                ("noise_kind", ctypes.c_int32), ("n_quantiles", ctypes.c_int32),
                ("scale", ctypes.c_double), ("quantiles", ctypes.c_double * 16),
                ("pk_offset", ctypes.c_int64), ("pk_stride", ctypes.c_int64),
                ("nonce", ctypes.c_uint64)]


class VectorParams(ctypes.Structure):
    """dpg_vector_params: the clip and the per-coordinate noise of VECTOR_SUM."""
    _fields_ = [("size", ctypes.c_int32), ("norm_kind", ctypes.c_int32),
                ("max_norm", ctypes.c_double),
                ("noise_kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("scale", ctypes.c_double),
                ("pk_offset", ctypes.c_int64), ("pk_stride", ctypes.c_int64),
                ("nonce", ctypes.c_uint64)]


class PairEntry(ctypes.Structure):
    """dpg_pair_entry: one (privacy id, partition) pair of the pre-aggregate."""
    _fields_ = [("pk", ctypes.c_uint32), ("count", ctypes.c_uint32), ("sum", ctypes.c_double),
                ("n_partitions", ctypes.c_uint32),
                ("contributions_leader", ctypes.c_uint32)]  # n_contributions | leader << 31


class HistOut(ctypes.Structure):
    """dpg_hist_out: device outputs of dpg_dataset_histograms."""
    _fields_ = [("int_bins", ctypes.c_void_p), ("sum_count", ctypes.c_void_p),
                ("sum_sum", ctypes.c_void_p), ("sum_max", ctypes.c_void_p),
                ("lowers", ctypes.c_void_p)]


class UaConfig(ctypes.Structure):
    _fields_ = [("max_partitions_contributed", ctypes.c_int64),
                ("max_contributions_per_partition", ctypes.c_int64),
                ("min_sum_per_partition", ctypes.c_double),
                ("max_sum_per_partition", ctypes.c_double),
                ("selection_strategy", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("pre_threshold", ctypes.c_int64), ("keep_table", ctypes.c_void_p),
                ("table_len", ctypes.c_int64), ("threshold", ctypes.c_double),
                ("noise_scale", ctypes.c_double), ("noise_std", ctypes.c_double * 3)]


class UaParams(ctypes.Structure):
    _fields_ = [("n_configs", ctypes.c_int32), ("metric_mask", ctypes.c_uint32),
                ("public_partitions", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("configs", ctypes.c_void_p), ("sample_mask", ctypes.c_void_p),
                ("public_mask", ctypes.c_void_p)]


def fill(struct_type, fields: dict):
    s = struct_type()
    for k, v in fields.items():
        if k in ("out_src", "quantiles") or (k == "scale" and not isinstance(v, float)):
            arr = getattr(s, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(s, k, v)
    return s


_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    pass


def library_path() -> str:
    return _LIB_PATH


def load():
    """Loads libdpg.so; raises NativeError if it was not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = os.environ.get("DPG_LIB_PATH") or _LIB_PATH  # debug: A/B builds
        if os.environ.get("DPG_PHASE_TIMING"):
            # debug build with per-phase cycle counters (tools/gpu_phase.sh)
            path = _LIB_PATH.replace("libdpg.so", "libdpg_timing.so")
        if not os.path.exists(path):
            raise NativeError(
                f"{path} is missing: build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'`. "
                f"There is no CPU fallback for the MI355X hot path.")
        lib = ctypes.CDLL(path)
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
        lib.dpg_ctx_create.argtypes = [ctypes.c_int, ctypes.c_uint64]
        lib.dpg_ctx_create.restype = vp
        lib.dpg_ctx_destroy.argtypes = [vp]
        lib.dpg_ctx_destroy.restype = None
        lib.dpg_last_error.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
        lib.dpg_last_error.restype = ctypes.c_int
        lib.dpg_set_seed.argtypes = [vp, ctypes.c_uint64]
        lib.dpg_set_seed.restype = ctypes.c_int
        lib.dpg_stream_seed.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
        lib.dpg_stream_seed.restype = ctypes.c_uint64
        lib.dpg_set_tuning.argtypes = [vp, i32, i32]
        lib.dpg_set_tuning.restype = ctypes.c_int
        lib.dpg_bound_aggregate.argtypes = [vp, vp, vp, vp, i64,
                                            ctypes.POINTER(BoundParams),
                                            ctypes.POINTER(Partials), vp]
        lib.dpg_bound_aggregate.restype = ctypes.c_int
        lib.dpg_select_and_noise.argtypes = [vp, ctypes.POINTER(Partials),
                                             ctypes.POINTER(SelectParams),
                                             ctypes.POINTER(NoiseParams), vp, vp, vp]
        lib.dpg_select_and_noise.restype = ctypes.c_int
        lib.dpg_compact_kept.argtypes = [vp, vp, vp, i64, i32, vp, vp,
                                         ctypes.POINTER(ctypes.c_int64), vp]
        lib.dpg_compact_kept.restype = ctypes.c_int
        lib.dpg_compact_kept_async.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, vp]
        lib.dpg_compact_kept_async.restype = ctypes.c_int
        lib.dpg_preaggregate.argtypes = [vp, vp, vp, vp, i64, ctypes.POINTER(BoundParams), vp,
                                         i64, vp, ctypes.POINTER(ctypes.c_int64), vp]
        lib.dpg_preaggregate.restype = ctypes.c_int
        lib.dpg_utility_analysis.argtypes = [vp, vp, vp, i64, ctypes.POINTER(UaParams), vp, vp,
                                             vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
        lib.dpg_utility_analysis.restype = ctypes.c_int
        lib.dpg_dataset_histograms.argtypes = [vp, vp, i64, vp, i64, i32,
                                               ctypes.POINTER(HistOut), vp]
        lib.dpg_dataset_histograms.restype = ctypes.c_int
        lib.dpg_hist_pairs.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]
        lib.dpg_hist_pairs.restype = ctypes.c_int
        lib.dpg_hist_partitions.argtypes = [vp, vp, vp, i64, vp, vp]
        lib.dpg_hist_partitions.restype = ctypes.c_int
        lib.dpg_hist_sums.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp]
        lib.dpg_hist_sums.restype = ctypes.c_int
        lib.dpg_last_stage_times.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.c_double), i32,
                                             ctypes.POINTER(ctypes.c_int32)]
        lib.dpg_last_stage_times.restype = ctypes.c_int
        lib.dpg_comm_unique_id.argtypes = [ctypes.c_char_p]
        lib.dpg_comm_unique_id.restype = ctypes.c_int
        lib.dpg_ctx_create_comm.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        lib.dpg_ctx_create_comm.restype = ctypes.c_int
        lib.dpg_reduce_scatter_partials.argtypes = [vp, ctypes.POINTER(Partials),
                                                    ctypes.POINTER(Partials),
                                                    ctypes.POINTER(ctypes.c_int64),
                                                    ctypes.POINTER(ctypes.c_int64), vp]
        lib.dpg_reduce_scatter_partials.restype = ctypes.c_int
        lib.dpg_pack_partials.argtypes = [vp, ctypes.POINTER(Partials), ctypes.c_int, vp, vp]
        lib.dpg_pack_partials.restype = ctypes.c_int
        lib.dpg_unpack_partials.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(Partials),
                                            ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int64), vp]
        lib.dpg_unpack_partials.restype = ctypes.c_int
        lib.dpg_export_error.argtypes = [vp, vp, vp]
        lib.dpg_export_error.restype = ctypes.c_int
        lib.dpg_import_error.argtypes = [vp, vp, i64, vp]
        lib.dpg_import_error.restype = ctypes.c_int
        lib.dpg_shard_records.argtypes = [vp, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp, vp]
        lib.dpg_shard_records.restype = ctypes.c_int
        lib.dpg_check_shard.argtypes = [vp, vp, i64, ctypes.c_int, ctypes.c_int, vp, vp]
        lib.dpg_check_shard.restype = ctypes.c_int
        lib.dpg_owner_split_keys.argtypes = [vp, vp, vp, i64, i32, ctypes.c_int, vp, vp, vp, vp]
        lib.dpg_owner_split_keys.restype = ctypes.c_int
        lib.dpg_owner_split_pairs.argtypes = [vp, vp, i64, ctypes.c_int, vp, vp, vp]
        lib.dpg_owner_split_pairs.restype = ctypes.c_int
        lib.dpg_merge_pair_runs.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                            i64, vp, vp, vp, vp]
        lib.dpg_merge_pair_runs.restype = ctypes.c_int
        lib.dpg_sort_pairs_u64.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp]
        lib.dpg_sort_pairs_u64.restype = ctypes.c_int
        lib.dpg_bound_records.argtypes = [vp, vp, vp, i64, ctypes.POINTER(BoundParams), vp, vp]
        lib.dpg_bound_records.restype = ctypes.c_int
        lib.dpg_quantile_keys.argtypes = [vp, vp, vp, vp, i64, i64,
                                          ctypes.POINTER(QuantileParams), vp, vp, vp]
        lib.dpg_quantile_keys.restype = ctypes.c_int
        lib.dpg_quantiles.argtypes = [vp, vp, vp, i64, ctypes.POINTER(QuantileParams), vp, vp, vp]
        lib.dpg_quantiles.restype = ctypes.c_int
        lib.dpg_vector_index.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp]
        lib.dpg_vector_index.restype = ctypes.c_int
        lib.dpg_vector_sums.argtypes = [vp, vp, vp, vp, i64, i32, i64, vp, vp]
        lib.dpg_vector_sums.restype = ctypes.c_int
        lib.dpg_vector_clip_noise.argtypes = [vp, vp, i64, ctypes.POINTER(VectorParams), vp, vp,
                                              vp]
        lib.dpg_vector_clip_noise.restype = ctypes.c_int
        lib.dpg_sample_partitions.argtypes = [vp, vp, i64, i64, i64, ctypes.c_uint64, i32, vp, vp,
                                              vp]
        lib.dpg_sample_partitions.restype = ctypes.c_int
        lib.dpg_partition_summary.argtypes = [vp, vp, i64, i64, vp, vp, vp]
        lib.dpg_partition_summary.restype = ctypes.c_int
        lib.dpg_keydict_insert.argtypes = [vp, vp, i64, vp, i64, vp, vp]
        lib.dpg_keydict_insert.restype = ctypes.c_int
        lib.dpg_keydict_keys.argtypes = [vp, vp, i64, vp, vp, vp]
        lib.dpg_keydict_keys.restype = ctypes.c_int
        lib.dpg_keydict_assign.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp]
        lib.dpg_keydict_assign.restype = ctypes.c_int
        lib.dpg_keydict_lookup.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, vp]
        lib.dpg_keydict_lookup.restype = ctypes.c_int
        lib.dpg_keydict_insert_slots.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
        lib.dpg_keydict_insert_slots.restype = ctypes.c_int
        lib.dpg_keydict_gather_ids.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
        lib.dpg_keydict_gather_ids.restype = ctypes.c_int
        lib.dpg_shard_records_wide.argtypes = lib.dpg_shard_records.argtypes
        lib.dpg_shard_records_wide.restype = ctypes.c_int
        lib.dpg_check_shard_wide.argtypes = lib.dpg_check_shard.argtypes
        lib.dpg_check_shard_wide.restype = ctypes.c_int
        lib.dpg_string_hash.argtypes = [vp, vp, vp, i64, i64, ctypes.c_uint64, vp, vp, vp]
        lib.dpg_string_hash.restype = ctypes.c_int
        lib.dpg_keydict_representatives.argtypes = [vp, vp, i64, i64, vp, vp]
        lib.dpg_keydict_representatives.restype = ctypes.c_int
        lib.dpg_string_verify.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp, vp]
        lib.dpg_string_verify.restype = ctypes.c_int
        lib.dpg_string_lengths.argtypes = [vp, vp, i64, i64, vp, i64, vp, vp, vp]
        lib.dpg_string_lengths.restype = ctypes.c_int
        lib.dpg_string_pack.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, i64, vp, vp]
        lib.dpg_string_pack.restype = ctypes.c_int
        lib.dpg_string_verify_runs.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp]
        lib.dpg_string_verify_runs.restype = ctypes.c_int
        _lib = lib
        return lib


def stream_seed(seed: int, nonce: int) -> int:
    """dpg_stream_seed: the key of every random stream of one release."""
    return int(load().dpg_stream_seed(ctypes.c_uint64(seed & (2**64 - 1)),
                                      ctypes.c_uint64(nonce & (2**64 - 1))))


class Context:
    """Owns one dpg_ctx (one device, one seed)."""

    def __init__(self, device: int, seed: int):
        self.lib = load()
        self.device = device
        self.handle = self.lib.dpg_ctx_create(int(device), ctypes.c_uint64(seed & (2**64 - 1)))
        if not self.handle:
            raise NativeError(f"dpg_ctx_create failed on device {device}")

    def close(self):
        if self.handle:
            self.lib.dpg_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, status: int, what: str):
        if status == DPG_OK:
            return
        buf = ctypes.create_string_buffer(1024)
        self.lib.dpg_last_error(self.handle, buf, 1024)
        msg = buf.value.decode(errors="replace")
        if status == 2:
            raise ValueError(f"{what}: {msg}")
        raise NativeError(f"{what} failed ({ERRORS.get(status, status)}): {msg}")

    def set_seed(self, seed: int):
        self.check(self.lib.dpg_set_seed(self.handle, ctypes.c_uint64(seed & (2**64 - 1))),
                   "dpg_set_seed")

    def set_tuning(self, bucket_target: int = 0, bucket_cap: int = 0):
        self.check(self.lib.dpg_set_tuning(self.handle, int(bucket_target), int(bucket_cap)),
                   "dpg_set_tuning")

    def bound_aggregate(self, pid_ptr, pk_ptr, value_ptr, n, bound: BoundParams,
                        partials: Partials, stream):
        st = self.lib.dpg_bound_aggregate(self.handle, pid_ptr, pk_ptr, value_ptr, n,
                                          ctypes.byref(bound), ctypes.byref(partials), stream)
        self.check(st, "dpg_bound_aggregate")

    def comm_unique_id(self) -> bytes:
        """RCCL unique id (rank 0), DPG_COMM_ID_BYTES opaque bytes."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        self.check(self.lib.dpg_comm_unique_id(buf), "dpg_comm_unique_id")
        return buf.raw

    def create_comm(self, uid: bytes, rank: int, nranks: int):
        self.check(self.lib.dpg_ctx_create_comm(self.handle, uid, rank, nranks),
                   "dpg_ctx_create_comm")

    def reduce_scatter_partials(self, full: Partials, slice_: Partials, stream):
        """Sums every rank's partials; this rank's slice (lo, n) lands in
        slice_ (see dpg.h)."""
        lo, n = ctypes.c_int64(0), ctypes.c_int64(0)
        st = self.lib.dpg_reduce_scatter_partials(self.handle, ctypes.byref(full),
                                                  ctypes.byref(slice_), ctypes.byref(lo),
                                                  ctypes.byref(n), stream)
        self.check(st, "dpg_reduce_scatter_partials")
        return lo.value, n.value

    def pack_partials(self, full: Partials, nranks: int, pack_ptr, stream):
        st = self.lib.dpg_pack_partials(self.handle, ctypes.byref(full), nranks, pack_ptr, stream)
        self.check(st, "dpg_pack_partials")

    def unpack_partials(self, part_ptr, n_partitions: int, nranks: int, rank: int,
                        slice_: Partials, stream):
        lo, n = ctypes.c_int64(0), ctypes.c_int64(0)
        st = self.lib.dpg_unpack_partials(self.handle, part_ptr, n_partitions, nranks, rank,
                                          ctypes.byref(slice_), ctypes.byref(lo),
                                          ctypes.byref(n), stream)
        self.check(st, "dpg_unpack_partials")
        return lo.value, n.value

    def export_error(self, dst_ptr, stream):
        """1.0 at device dst if the last bounding latched an internal error."""
        self.check(self.lib.dpg_export_error(self.handle, dst_ptr, stream), "dpg_export_error")

    def import_error(self, src_ptr, n: int, stream):
        """Latches the internal error if any of n device doubles is nonzero
        (the next compact then fails)."""
        self.check(self.lib.dpg_import_error(self.handle, src_ptr, n, stream), "dpg_import_error")

    def shard_records(self, pid_ptr, pk_ptr, value_ptr, n, nranks, out_pid_ptr, out_pk_ptr,
                      out_value_ptr, counts_ptr, stream):
        """Stable split of n records by distributed.shard_of(pid, nranks) into
        the out arrays, destination-major; counts (device int64[nranks])."""
        st = self.lib.dpg_shard_records(self.handle, pid_ptr, pk_ptr, value_ptr, n, nranks,
                                        out_pid_ptr, out_pk_ptr, out_value_ptr, counts_ptr, stream)
        self.check(st, "dpg_shard_records")

    def check_shard(self, pid_ptr, n, nranks, rank, n_bad_ptr, stream):
        """Device int64 at n_bad_ptr = records whose owner is not `rank`."""
        st = self.lib.dpg_check_shard(self.handle, pid_ptr, n, nranks, rank, n_bad_ptr, stream)
        self.check(st, "dpg_check_shard")

    def shard_records_wide(self, pid_ptr, pk_ptr, value_ptr, n, nranks, out_pid_ptr, out_pk_ptr,
                           out_value_ptr, counts_ptr, stream):
        """shard_records by distributed.shard_of_wide(pid, nranks): the owner
        of a wide privacy id (ColumnarData(wide_privacy_ids=True))."""
        st = self.lib.dpg_shard_records_wide(self.handle, pid_ptr, pk_ptr, value_ptr, n, nranks,
                                             out_pid_ptr, out_pk_ptr, out_value_ptr, counts_ptr,
                                             stream)
        self.check(st, "dpg_shard_records_wide")

    def check_shard_wide(self, pid_ptr, n, nranks, rank, n_bad_ptr, stream):
        """check_shard by distributed.shard_of_wide."""
        st = self.lib.dpg_check_shard_wide(self.handle, pid_ptr, n, nranks, rank, n_bad_ptr,
                                           stream)
        self.check(st, "dpg_check_shard_wide")

    def owner_split_keys(self, keys_ptr, n_keys_ptr, n_max, low_bits, nranks, out_keys_ptr,
                         out_src_ptr, counts_ptr, stream):
        """Stable split of the first *n_keys_ptr (device int64) keys by the
        owner (key >> low_bits) % nranks into out_keys, destination-major and
        re-based to the owner's local partition ids; out_src (or None): the
        input positions; counts (device int64[nranks])."""
        st = self.lib.dpg_owner_split_keys(self.handle, keys_ptr, n_keys_ptr, n_max, low_bits,
                                           nranks, out_keys_ptr, out_src_ptr, counts_ptr, stream)
        self.check(st, "dpg_owner_split_keys")

    def owner_split_pairs(self, pairs_ptr, n, nranks, out_pairs_ptr, counts_ptr, stream):
        """Stable split of n dpg_pair_entry by the owner pk % nranks into
        out_pairs, destination-major, pk re-based to the owner's local
        partition ids (pk // nranks); counts (device int64[nranks])."""
        st = self.lib.dpg_owner_split_pairs(self.handle, pairs_ptr, n, nranks, out_pairs_ptr,
                                            counts_ptr, stream)
        self.check(st, "dpg_owner_split_pairs")

    def merge_pair_runs(self, pairs_ptr, run_start, n_partitions, out_pairs_ptr, starts_ptr,
                        n_bad_ptr, stream):
        """Merges the pk-sorted runs [run_start[r], run_start[r + 1]) (host
        ints) of dpg_pair_entry into out_pairs, ascending by pk, then run,
        then position; starts (device int64[n_partitions + 1]); the device
        int64 at n_bad_ptr counts out-of-range and descending entries."""
        rs = (ctypes.c_int64 * len(run_start))(*[int(x) for x in run_start])
        st = self.lib.dpg_merge_pair_runs(self.handle, pairs_ptr, rs, len(run_start) - 1,
                                          n_partitions, out_pairs_ptr, starts_ptr, n_bad_ptr,
                                          stream)
        self.check(st, "dpg_merge_pair_runs")

    def sort_pairs_u64(self, keys_in_ptr, vals_in_ptr, n, begin_bit, end_bit, keys_out_ptr,
                       vals_out_ptr, stream):
        """Stable radix sort of n (uint64 key, uint32 payload) pairs by the key
        bits [begin_bit, end_bit); the payload pointers may both be None."""
        st = self.lib.dpg_sort_pairs_u64(self.handle, keys_in_ptr, vals_in_ptr, n, begin_bit,
                                         end_bit, keys_out_ptr, vals_out_ptr, stream)
        self.check(st, "dpg_sort_pairs_u64")

    def bound_records(self, pid_ptr, pk_ptr, n, bound: BoundParams, keep_ptr, stream):
        """Device uint8[n] at keep_ptr: 1 for the records dpg_bound_aggregate
        keeps under the same seed and params."""
        st = self.lib.dpg_bound_records(self.handle, pid_ptr, pk_ptr, n, ctypes.byref(bound),
                                        keep_ptr, stream)
        self.check(st, "dpg_bound_records")

    def quantile_keys(self, pk_ptr, value_ptr, keep_ptr, n, n_partitions, q: QuantileParams,
                      keys_ptr, n_keys_ptr, stream):
        """Sorted tree keys (pk << 16 | leaf) of the kept, non-NaN records."""
        st = self.lib.dpg_quantile_keys(self.handle, pk_ptr, value_ptr, keep_ptr, n, n_partitions,
                                        ctypes.byref(q), keys_ptr, n_keys_ptr, stream)
        self.check(st, "dpg_quantile_keys")

    def quantiles(self, keys_ptr, n_keys_ptr, n_partitions, q: QuantileParams,
                  keep_partition_ptr, out_ptr, stream):
        """Device double[P][n_quantiles] at out_ptr from the noised trees."""
        st = self.lib.dpg_quantiles(self.handle, keys_ptr, n_keys_ptr, n_partitions,
                                    ctypes.byref(q), keep_partition_ptr, out_ptr, stream)
        self.check(st, "dpg_quantiles")

    def vector_index(self, pk_ptr, keep_ptr, n, n_partitions, keys_ptr, n_keys_ptr, stream):
        """Sorted keys (pk << 31 | record index) of the kept records."""
        st = self.lib.dpg_vector_index(self.handle, pk_ptr, keep_ptr, n, n_partitions, keys_ptr,
                                       n_keys_ptr, stream)
        self.check(st, "dpg_vector_index")

    def vector_sums(self, keys_ptr, n_keys_ptr, value_ptr, n, size, n_partitions, out_ptr, stream):
        """Device double[P][size] at out_ptr: the per-partition sums of the
        indexed rows of value (double[n][size]), in a fixed order."""
        st = self.lib.dpg_vector_sums(self.handle, keys_ptr, n_keys_ptr, value_ptr, n, size,
                                      n_partitions, out_ptr, stream)
        self.check(st, "dpg_vector_sums")

    def vector_clip_noise(self, sums_ptr, n_partitions, v: VectorParams, keep_partition_ptr,
                          out_ptr, stream):
        """Clips every kept partition's summed vector and noises its coordinates."""
        st = self.lib.dpg_vector_clip_noise(self.handle, sums_ptr, n_partitions, ctypes.byref(v),
                                            keep_partition_ptr, out_ptr, stream)
        self.check(st, "dpg_vector_clip_noise")

    def select_and_noise(self, partials: Partials, sel: SelectParams, noise: NoiseParams,
                         keep_ptr, out_ptr, stream):
        st = self.lib.dpg_select_and_noise(self.handle, ctypes.byref(partials),
                                           ctypes.byref(sel), ctypes.byref(noise),
                                           keep_ptr, out_ptr, stream)
        self.check(st, "dpg_select_and_noise")

    def compact(self, keep_ptr, out_ptr, n_partitions, n_out, ids_ptr, kept_out_ptr, stream) -> int:
        n = ctypes.c_int64(0)
        st = self.lib.dpg_compact_kept(self.handle, keep_ptr, out_ptr, n_partitions, n_out,
                                       ids_ptr, kept_out_ptr, ctypes.byref(n), stream)
        self.check(st, "dpg_compact_kept")
        return n.value

    def compact_async(self, keep_ptr, out_ptr, n_partitions, n_out, ids_ptr, kept_out_ptr,
                      info_ptr, stream) -> None:
        """dpg_compact_kept without the host synchronisation: the kept count
        and the bounding's error bits land in the device int64[2] at
        info_ptr in stream order."""
        st = self.lib.dpg_compact_kept_async(self.handle, keep_ptr, out_ptr, n_partitions, n_out,
                                             ids_ptr, kept_out_ptr, info_ptr, stream)
        self.check(st, "dpg_compact_kept_async")

    def preaggregate(self, pid_ptr, pk_ptr, value_ptr, n, bound: BoundParams, pairs_ptr,
                     capacity, starts_ptr, stream) -> int:
        n_pairs = ctypes.c_int64(0)
        st = self.lib.dpg_preaggregate(self.handle, pid_ptr, pk_ptr, value_ptr, n,
                                       ctypes.byref(bound), pairs_ptr, capacity, starts_ptr,
                                       ctypes.byref(n_pairs), stream)
        self.check(st, "dpg_preaggregate")
        return n_pairs.value

    def utility_analysis(self, pairs_ptr, starts_ptr, n_partitions, params: UaParams, raw_ptr,
                         err_ptr, keep_ptr, report_ptr, stream) -> int:
        n_out = ctypes.c_int64(0)
        st = self.lib.dpg_utility_analysis(self.handle, pairs_ptr, starts_ptr, n_partitions,
                                           ctypes.byref(params), raw_ptr, err_ptr, keep_ptr,
                                           report_ptr, ctypes.byref(n_out), stream)
        self.check(st, "dpg_utility_analysis")
        return n_out.value

    def dataset_histograms(self, pairs_ptr, n_pairs, starts_ptr, n_partitions,
                           pre_aggregated: bool, out: HistOut, stream):
        st = self.lib.dpg_dataset_histograms(self.handle, pairs_ptr, n_pairs, starts_ptr,
                                             n_partitions, int(bool(pre_aggregated)),
                                             ctypes.byref(out), stream)
        self.check(st, "dpg_dataset_histograms")

    def hist_pairs(self, pairs_ptr, n_pairs, starts_ptr, n_partitions, int_bins_ptr,
                   part_rows_ptr, part_count_ptr, sum_range_ptr, stream):
        """Phase 1 of the histograms: L0 / L1 / LINF into int_bins (zero-filled),
        the pairs and records per partition (device int64[n_partitions] each)
        and the (min, max) pair sum (device double[2])."""
        st = self.lib.dpg_hist_pairs(self.handle, pairs_ptr, n_pairs, starts_ptr, n_partitions,
                                     int_bins_ptr, part_rows_ptr, part_count_ptr, sum_range_ptr,
                                     stream)
        self.check(st, "dpg_hist_pairs")

    def hist_partitions(self, rows_ptr, count_ptr, n, int_bins_ptr, stream):
        """Phase 2: adds the per-partition histograms of n partitions' totals."""
        st = self.lib.dpg_hist_partitions(self.handle, rows_ptr, count_ptr, n, int_bins_ptr,
                                          stream)
        self.check(st, "dpg_hist_partitions")

    def hist_sums(self, pairs_ptr, n_pairs, sum_range_ptr, sum_count_ptr, sum_sum_ptr,
                  sum_max_ptr, lowers_ptr, stream):
        """Phase 3: LINF_SUM of these pairs between the edges of the given range."""
        st = self.lib.dpg_hist_sums(self.handle, pairs_ptr, n_pairs, sum_range_ptr,
                                    sum_count_ptr, sum_sum_ptr, sum_max_ptr, lowers_ptr, stream)
        self.check(st, "dpg_hist_sums")

    def sample_partitions(self, keys_ptr, key_lo, key_stride, n, bound: int, mask_ptr,
                          hashes_ptr, stream):
        """Device bitmap at mask_ptr (8 * ceil(n / 64) bytes) of the keys whose
        sampler hash is below bound (an int in [0, 2^64]; 2^64 keeps all);
        keys_ptr None: the keys key_lo + i * key_stride.  Stream-ordered."""
        keep_all = bound >= 2**64
        st = self.lib.dpg_sample_partitions(self.handle, keys_ptr, int(key_lo), int(key_stride),
                                            int(n), ctypes.c_uint64(0 if keep_all else bound),
                                            int(keep_all), mask_ptr, hashes_ptr, stream)
        self.check(st, "dpg_sample_partitions")

    def partition_summary(self, pk_ptr, n, n_partitions, public_mask_ptr, counts_ptr, stream):
        """Device int64[3] at counts_ptr: partitions present and public,
        present and not public, public and not present."""
        st = self.lib.dpg_partition_summary(self.handle, pk_ptr, int(n), int(n_partitions),
                                            public_mask_ptr, counts_ptr, stream)
        self.check(st, "dpg_partition_summary")

    def keydict_insert(self, keys_ptr, n, slots_ptr, capacity, info_ptr, stream):
        """Inserts the distinct values of n int64 keys into the write-once
        table slots (device uint64[capacity], filled with KEYDICT_EMPTY);
        info (device int64[2]) += (records with the reserved key INT64_MIN,
        records that found no slot)."""
        st = self.lib.dpg_keydict_insert(self.handle, keys_ptr, int(n), slots_ptr, int(capacity),
                                         info_ptr, stream)
        self.check(st, "dpg_keydict_insert")

    def keydict_keys(self, slots_ptr, capacity, out_keys_ptr, n_keys_ptr, stream):
        """The occupied slots' keys, compacted into out_keys (device
        int64[capacity], unspecified order); their count at n_keys_ptr."""
        st = self.lib.dpg_keydict_keys(self.handle, slots_ptr, int(capacity), out_keys_ptr,
                                       n_keys_ptr, stream)
        self.check(st, "dpg_keydict_keys")

    def keydict_assign(self, keys_ptr, ids_ptr, n, slots_ptr, slot_ids_ptr, capacity,
                       n_missing_ptr, stream):
        """slot_ids[slot of keys[i]] = ids[i] (device int64, < 2^32 - 1); the
        device int64 at n_missing_ptr += keys that are not in the table."""
        st = self.lib.dpg_keydict_assign(self.handle, keys_ptr, ids_ptr, int(n), slots_ptr,
                                         slot_ids_ptr, int(capacity), n_missing_ptr, stream)
        self.check(st, "dpg_keydict_assign")

    def keydict_lookup(self, keys_ptr, n, slots_ptr, slot_ids_ptr, capacity, out_ids_ptr,
                       n_missing_ptr, stream):
        """out_ids[i] (device int64) = the id assigned to keys[i], -1 for an
        absent or reserved key, which the device int64 at n_missing_ptr counts."""
        st = self.lib.dpg_keydict_lookup(self.handle, keys_ptr, int(n), slots_ptr, slot_ids_ptr,
                                         int(capacity), out_ids_ptr, n_missing_ptr, stream)
        self.check(st, "dpg_keydict_lookup")

    def keydict_insert_slots(self, keys_ptr, n, slots_ptr, capacity, out_slots_ptr, info_ptr,
                             stream):
        """keydict_insert that also stores every record's final slot in
        out_slots (device uint32[n]); KEYDICT_NO_SLOT for a record that holds
        the reserved key or found no slot."""
        st = self.lib.dpg_keydict_insert_slots(self.handle, keys_ptr, int(n), slots_ptr,
                                               int(capacity), out_slots_ptr, info_ptr, stream)
        self.check(st, "dpg_keydict_insert_slots")

    def keydict_gather_ids(self, out_slots_ptr, n, slot_ids_ptr, capacity, out_ids_ptr,
                           n_missing_ptr, stream):
        """out_ids[i] (device int64) = slot_ids[out_slots[i]]; KEYDICT_NO_SLOT
        gives -1, which the device int64 at n_missing_ptr counts."""
        st = self.lib.dpg_keydict_gather_ids(self.handle, out_slots_ptr, int(n), slot_ids_ptr,
                                             int(capacity), out_ids_ptr, n_missing_ptr, stream)
        self.check(st, "dpg_keydict_gather_ids")

    def string_hash(self, offsets_ptr, data_ptr, data_len, n, seed, out_keys_ptr, info_ptr,
                    stream):
        """out_keys[i] (device int64) = the 64-bit key of the string
        data[offsets[i]:offsets[i + 1]] (the definition is in dpg.h); a record
        with offsets outside 0 <= start <= end <= data_len gets key 0 and the
        device int64 at info_ptr += 1."""
        st = self.lib.dpg_string_hash(self.handle, offsets_ptr, data_ptr, int(data_len), int(n),
                                      ctypes.c_uint64(int(seed) & (2**64 - 1)), out_keys_ptr,
                                      info_ptr, stream)
        self.check(st, "dpg_string_hash")

    def keydict_representatives(self, rec_slots_ptr, n, capacity, rep_ptr, stream):
        """rep[s] (device uint32[capacity], filled with KEYDICT_NO_SLOT) = the
        smallest i with rec_slots[i] == s."""
        st = self.lib.dpg_keydict_representatives(self.handle, rec_slots_ptr, int(n),
                                                  int(capacity), rep_ptr, stream)
        self.check(st, "dpg_keydict_representatives")

    def string_verify(self, offsets_ptr, data_ptr, data_len, n, rec_slots_ptr, rep_ptr,
                      n_mismatch_ptr, stream):
        """The device int64 at n_mismatch_ptr += records whose bytes differ
        from those of their slot's representative rep[rec_slots[i]]."""
        st = self.lib.dpg_string_verify(self.handle, offsets_ptr, data_ptr, int(data_len), int(n),
                                        rec_slots_ptr, rep_ptr, n_mismatch_ptr, stream)
        self.check(st, "dpg_string_verify")

    def string_lengths(self, offsets_ptr, data_len, n, records_ptr, m, out_len_ptr, info_ptr,
                       stream):
        """out_len[j] (device int64[m]) = the byte length of record records[j]
        of an n-record column; an invalid record or invalid offsets give 0 and
        the device int64 at info_ptr += 1."""
        st = self.lib.dpg_string_lengths(self.handle, offsets_ptr, int(data_len), int(n),
                                         records_ptr, int(m), out_len_ptr, info_ptr, stream)
        self.check(st, "dpg_string_lengths")

    def string_pack(self, offsets_ptr, data_ptr, data_len, n, records_ptr, m, out_offsets_ptr,
                    out_data_ptr, out_total, info_ptr, stream):
        """out_data[out_offsets[j]:out_offsets[j + 1]] = the bytes of record
        records[j]; a j that is invalid or whose out range does not fit writes
        nothing and the device int64 at info_ptr += 1."""
        st = self.lib.dpg_string_pack(self.handle, offsets_ptr, data_ptr, int(data_len), int(n),
                                      records_ptr, int(m), out_offsets_ptr, out_data_ptr,
                                      int(out_total), info_ptr, stream)
        self.check(st, "dpg_string_pack")

    def string_verify_runs(self, keys_ptr, order_ptr, offsets_ptr, data_ptr, data_len, n_strings,
                           m, head_ptr, info_ptr, stream):
        """head[j] (device uint8[m]) = keys[j] starts a run of equal keys; any
        other entry's string order[j] (order_ptr None: j) is compared with its
        predecessor's: info (device int64[2]) += (differences, of which
        invalid indices or offsets)."""
        st = self.lib.dpg_string_verify_runs(self.handle, keys_ptr, order_ptr, offsets_ptr,
                                             data_ptr, int(data_len), int(n_strings), int(m),
                                             head_ptr, info_ptr, stream)
        self.check(st, "dpg_string_verify_runs")

    def stage_times(self):
        names = ctypes.create_string_buffer(4096)
        ms = (ctypes.c_double * 64)()
        ns = ctypes.c_int32(0)
        self.check(self.lib.dpg_last_stage_times(self.handle, names, 4096, ms, 64,
                                                 ctypes.byref(ns)), "stage_times")
        keys = names.value.decode().split(",") if ns.value else []
        return dict(zip(keys, [ms[i] for i in range(ns.value)]))
