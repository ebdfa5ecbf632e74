/*
 * dpg.h -- C ABI of the MI355X-native DPEngine.aggregate hot path
 *          (libdpg.so, built from the HIP sources in pipelinedp_amd/csrc for gfx950).
 *
 * Plain pointers and sizes only; no torch or HIP types in the signatures
 * (streams travel as void*).  Every entry point returns an int status
 * (DPG_OK = 0) and never throws across the ABI; dpg_last_error() returns
 * the message of the last failure on a context.  One context per
 * (host thread, device); calls on one context are not re-entrant.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * PipelineDP reference tree):
 *   dpg_bound_aggregate  <- DPEngine._aggregate up to the partition merge:
 *        pipeline_dp/dp_engine.py:113-151 (extract, drop public, bound,
 *        drop pid, add empty public, combine_accumulators_per_key), i.e.
 *        contribution_bounders.py:66-195 + combiners.py:691-706 +
 *        pipeline_backend.py:531-565 (LocalBackend sample/group/reduce).
 *   dpg_select_and_noise <- DPEngine._select_private_partitions_internal
 *        (dp_engine.py:305-361, PyDP create_partition_strategy().should_keep)
 *        fused with CompoundCombiner.compute_metrics (combiners.py:708-730,
 *        dp_computations.py:120-184, 307-366, 541-576; PyDP add_noise).
 *   dpg_compact_kept     <- the LocalBackend `filter` materialisation
 *        (pipeline_backend.py:514-515) of the selected partitions.
 *   dpg_preaggregate     <- utility analysis' per-(privacy id, partition)
 *        pre-aggregation: analysis/contribution_bounders.py:37-77
 *        (AnalysisContributionBounder) and analysis/pre_aggregation.py:19-61.
 *   dpg_utility_analysis <- the per-partition utility combiners of every
 *        configuration of a sweep: analysis/per_partition_combiners.py:195-356
 *        (PartitionSelection / Sum / Count / PrivacyIdCount / RawStatistics)
 *        with analysis/poisson_binomial.py:39-83, driven by
 *        analysis/utility_analysis_engine.py:98-143.
 *   dpg_dataset_histograms <- pipeline_dp/dataset_histograms/
 *        computing_histograms.py:420-474 (compute_dataset_histograms, over
 *        the dpg_preaggregate pairs) and :642-684
 *        (compute_dataset_histograms_on_preaggregated_data), which feed
 *        DPEngine.calculate_private_contribution_bounds (dp_engine.py:432-484)
 *        and analysis/parameter_tuning.py:278-348 (tune).
 *   dpg_bound_records / dpg_quantile_keys / dpg_quantiles <- QuantileCombiner
 *        (pipeline_dp/combiners.py:532-611: PyDP QuantileTree per
 *        (privacy id, partition) accumulator, merged per partition, then
 *        compute_quantiles) on the records contribution bounding keeps
 *        (contribution_bounders.py:66-105).
 *   dpg_vector_index / dpg_vector_sums / dpg_vector_clip_noise <-
 *        VectorSumCombiner (pipeline_dp/combiners.py: the per-partition sum of
 *        the kept records' vectors) with dp_computations.py _clip_vector and
 *        add_noise_vector at the release.
 */
#ifndef DPG_H_
#define DPG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define DPG_OK 0
#define DPG_ERR_INVALID_ARG 1
#define DPG_ERR_KEY_RANGE 2   /* pid outside its declared range or pk outside [0, P) */
#define DPG_ERR_HIP 3
#define DPG_ERR_OOM 4
#define DPG_ERR_UNSUPPORTED 5

/* ---- Philox key tags: domain separation of the keyed random streams ---- */
#define DPG_TAG_PAIR 0x50414952u   /* pair priority      (pid, pk)              */
#define DPG_TAG_REC 0x52454344u    /* record priority    (pid, pk, record id)   */
#define DPG_TAG_SELECT 0x53454C45u /* partition selection (pk)                  */
#define DPG_TAG_NOISE 0x4E4F4953u  /* metric noise        (pk, slot)            */

/* ---- contribution-bounding modes (dp_engine.py:370-382) ---- */
#define DPG_MODE_CROSS_AND_PER_PARTITION 0 /* SamplingCrossAndPerPartition   */
#define DPG_MODE_PER_PRIVACY_ID 1          /* SamplingPerPrivacyId (L1)      */
#define DPG_MODE_CROSS_PARTITION 2         /* SamplingCrossPartition         */

/* ---- how SUM is bounded (combiners.py:348-353) ---- */
#define DPG_SUM_NONE 0
#define DPG_SUM_CLIP_VALUE 1     /* clip every value to [min_value, max_value] */
#define DPG_SUM_CLIP_PARTITION 2 /* clip the per-(pid,pk) sum                   */

/* ---- accumulator mask ---- */
#define DPG_M_COUNT 1u
#define DPG_M_SUM 2u
#define DPG_M_PRIVACY_ID_COUNT 4u
#define DPG_M_MEAN 8u
#define DPG_M_VARIANCE 16u

/* ---- partition selection (partition_selection.py:19-44) ---- */
#define DPG_SELECT_NONE 0 /* public partitions: keep iff in public_mask */
#define DPG_SELECT_TRUNCATED_GEOMETRIC 1
#define DPG_SELECT_LAPLACE_THRESHOLD 2
#define DPG_SELECT_GAUSSIAN_THRESHOLD 3

/* ---- noise ---- */
#define DPG_NOISE_NONE 0
#define DPG_NOISE_LAPLACE 1
#define DPG_NOISE_GAUSSIAN 2

#define DPG_FAMILY_SCALAR 0   /* Count / Sum / PrivacyIdCount combiners    */
#define DPG_FAMILY_MEAN 1     /* MeanCombiner (+ PrivacyIdCount)           */
#define DPG_FAMILY_VARIANCE 2 /* VarianceCombiner (+ PrivacyIdCount)       */

/* noise slots (each gets its own Philox counter) */
#define DPG_SLOT_COUNT 0
#define DPG_SLOT_SUM 1 /* SUM, or the normalised sum of MEAN/VARIANCE */
#define DPG_SLOT_NSQ 2 /* normalised sum of squares (VARIANCE)        */
#define DPG_SLOT_PID 3 /* PRIVACY_ID_COUNT                             */
/* quantile tree: node nu of a partition draws from slot DPG_SLOT_QNODE0 + nu
 * (root = node 0, children of node i = 16 i + 1 .. 16 i + 16) */
#define DPG_SLOT_QNODE0 16
/* VECTOR_SUM: coordinate d of a partition draws from slot DPG_SLOT_VEC0 + d
 * (clear of DPG_SLOT_QNODE0 + node, which stays below 69921) */
#define DPG_SLOT_VEC0 (1u << 20)

/* value-vector entries an output column can be mapped from */
#define DPG_V_COUNT 0
#define DPG_V_SUM 1
#define DPG_V_MEAN 2
#define DPG_V_VARIANCE 3
#define DPG_V_PRIVACY_ID_COUNT 4

typedef struct dpg_bound_params {
    int32_t mode;        /* DPG_MODE_*                               */
    int32_t sum_mode;    /* DPG_SUM_*                                */
    uint32_t metric_mask;/* DPG_M_* accumulators to produce          */
    int32_t reserved0;
    int64_t max_partitions_contributed;      /* mpc (l0)            */
    int64_t max_contributions_per_partition; /* mcpp (linf)         */
    int64_t max_contributions;               /* L1 (PER_PRIVACY_ID) */
    double min_value, max_value;
    double min_sum_per_partition, max_sum_per_partition;
    int64_t n_partitions;        /* P: pk ids are dense in [0, P)   */
    const uint8_t *public_mask;  /* bitmap of P bits (device memory for
                                    libdpg, host memory for the oracle);
                                    NULL = private partition selection */
    int64_t pid_min;             /* privacy ids lie in [pid_min,        */
    int64_t pid_count;           /*   pid_min + pid_count); pid_count <= 2^32.
                                    0 = unknown: libdpg reduces min/max on
                                    the device first                     */
    int64_t rec_id_offset;       /* global id of input record 0: the
                                    record sampler is keyed by
                                    (pid, pk, rec_id_offset + i), so shards
                                    of one dataset sample as the whole   */
    uint64_t nonce;              /* per-release nonce: every keyed stream of
                                    the call uses dpg_stream_seed(ctx seed,
                                    nonce).  Callers pass a FRESH random
                                    nonce per release (the reference draws
                                    fresh randomness per call,
                                    dp_computations.py:131-133, 151-152,
                                    pipeline_backend.py:540-544) and the
                                    same nonce on every rank of one release */
} dpg_bound_params;

/* Dense per-partition partial accumulators (structure of arrays).
 * rows  = number of kept (privacy id, partition) pairs = privacy id count
 * count = number of kept records; sum = bounded sum;
 * nsum  = sum(clip(v) - mid), nsq = sum((clip(v) - mid)^2)
 * Unused float arrays may be NULL. */
typedef struct dpg_partials {
    int64_t n_partitions;
    int64_t *rows;
    int64_t *count;
    double *sum;
    double *nsum;
    double *nsq;
} dpg_partials;

typedef struct dpg_select_params {
    int32_t strategy;            /* DPG_SELECT_*                          */
    int32_t table_len;           /* truncated geometric: len(keep_table)  */
    const double *keep_table;    /* host pointer; pi(n) for n < table_len,
                                    1.0 beyond                              */
    double threshold;            /* Laplace/Gaussian thresholding          */
    double noise_scale;          /* b (Laplace) or sigma (Gaussian)        */
    int64_t pre_threshold;       /* 0 = none                               */
    int64_t max_rows_per_privacy_id; /* dp_engine.py:156-164 (normally 1)  */
    int64_t pk_offset;           /* global pk id of partials index 0       */
    const uint8_t *public_mask;  /* DPG_SELECT_NONE: keep iff bit set
                                    (indexed by local partition id)        */
    uint64_t nonce;              /* per-release nonce of the selection and
                                    noise draws (see dpg_bound_params)      */
    int64_t pk_stride;           /* global pk of partials index i is
                                    pk_offset + i * pk_stride (multi-GPU
                                    slices are interleaved: rank r owns
                                    r, r + R, ...); <= 0 means 1            */
} dpg_select_params;

typedef struct dpg_noise_params {
    int32_t noise_kind;  /* DPG_NOISE_*                                  */
    int32_t family;      /* DPG_FAMILY_*                                 */
    uint32_t slot_mask;  /* bit s: slot s exists (SCALAR / pid slot)     */
    int32_t n_outputs;   /* output columns per partition                 */
    int32_t out_src[8];  /* column j <- value vector entry DPG_V_*       */
    double scale[4];     /* per-slot noise scale: b or sigma             */
    double mid;          /* MEAN/VARIANCE range middle                   */
    int32_t mean_const;  /* VARIANCE: min_value == max_value             */
    int32_t msq_const;   /* VARIANCE: squares interval degenerate        */
    double mean_const_value;
    double msq_const_value;
} dpg_noise_params;

/* One (privacy id, partition) pair of the utility-analysis pre-aggregate
 * (24 bytes): the pair's record count and value sum, the number of
 * partitions its privacy id contributes to and the privacy id's records.
 * Bit 31 of contributions_leader is the leader flag (dpg_preaggregate sets
 * it on one pair per privacy id); bits 0-30 are n_contributions. */
typedef struct dpg_pair_entry {
    uint32_t pk;
    uint32_t count;
    double sum;
    uint32_t n_partitions;
    uint32_t contributions_leader;  /* n_contributions | leader << 31 */
} dpg_pair_entry;

/* One row of a MultiParameterConfiguration (analysis/data_structures.py
 * :24-103) with the budget of its mechanisms resolved. */
typedef struct dpg_ua_config {
    int64_t max_partitions_contributed;      /* l0                          */
    int64_t max_contributions_per_partition; /* linf of COUNT               */
    double min_sum_per_partition;            /* SUM clipping                */
    double max_sum_per_partition;
    int32_t selection_strategy;  /* DPG_SELECT_* (private partitions)      */
    int32_t reserved;
    int64_t pre_threshold;       /* 0 = none                               */
    const double *keep_table;    /* host: truncated geometric pi(n)        */
    int64_t table_len;
    double threshold;            /* Laplace / Gaussian thresholding        */
    double noise_scale;
    double noise_std[3];         /* report: noise std of SUM, COUNT and
                                    PRIVACY_ID_COUNT (compute_dp_count_noise_std,
                                    dp_computations.py:369-395)             */
} dpg_ua_config;

typedef struct dpg_ua_params {
    int32_t n_configs;           /* 1..64                                   */
    uint32_t metric_mask;        /* DPG_M_SUM | DPG_M_COUNT | DPG_M_PRIVACY_ID_COUNT */
    int32_t public_partitions;   /* 1: public partitions (no selection)    */
    int32_t reserved;
    const dpg_ua_config *configs;/* host [n_configs]                       */
    const uint8_t *sample_mask;  /* device bitmap of the partitions kept by
                                    partitions_sampling_prob, or NULL       */
    const uint8_t *public_mask;  /* device bitmap of public partitions     */
} dpg_ua_params;

/* Dataset histograms (pipeline_dp/dataset_histograms/histograms.py:60-75).
 * Integer histograms (L0, L1, LINF, COUNT_PER_PARTITION,
 * PRIVACY_ID_PER_PARTITION, in this order) have DPG_HIST_INT_BINS bins of 3
 * significant digits: bin v for v < 1000 ([v, v+1)), else
 * 1000 + 900 e + (m - 100) for [m 10^(e+1), (m+1) 10^(e+1)), m in [100, 999].
 * LINF_SUM has DPG_HIST_SUM_BINS equal bins between the smallest and the
 * largest pair sum; lowers[i] = np.linspace(min, max, bins + 1)[i]. */
#define DPG_HIST_INT_BINS 16300
#define DPG_HIST_SUM_BINS 10000
#define DPG_HIST_L0 0
#define DPG_HIST_L1 1
#define DPG_HIST_LINF 2
#define DPG_HIST_COUNT_PER_PARTITION 3
#define DPG_HIST_PRIVACY_ID_PER_PARTITION 4

typedef struct dpg_hist_out {
    uint64_t *int_bins;  /* device [5][DPG_HIST_INT_BINS][3]: count, sum, max;
                            a bin exists iff count > 0 or max > 0            */
    uint64_t *sum_count; /* device [DPG_HIST_SUM_BINS] LINF_SUM counts       */
    double *sum_sum;     /* device [DPG_HIST_SUM_BINS] LINF_SUM sums         */
    double *sum_max;     /* device [DPG_HIST_SUM_BINS] LINF_SUM maxima       */
    double *lowers;      /* device [DPG_HIST_SUM_BINS + 1] LINF_SUM lowers   */
} dpg_hist_out;

typedef struct dpg_ctx dpg_ctx;

/* Context: device ordinal and the 64-bit seed of every keyed random stream.
 * Returns NULL on failure. */
dpg_ctx *dpg_ctx_create(int device, uint64_t seed);
void dpg_ctx_destroy(dpg_ctx *ctx);
int dpg_last_error(dpg_ctx *ctx, char *buf, size_t len);
int dpg_set_seed(dpg_ctx *ctx, uint64_t seed);

/* The 64-bit key of every keyed random stream of one release:
 * mix64(seed ^ mix64(nonce + 0x9E3779B97F4A7C15)) with mix64 the SplitMix64
 * finaliser.  Two releases with different nonces draw independent sampling,
 * selection and noise; the same (seed, nonce) reproduces a release exactly
 * (tests, and every rank of one multi-GPU release). */
uint64_t dpg_stream_seed(uint64_t seed, uint64_t nonce);

/* Tuning / testing hook: average records per fine privacy-id bucket the
 * partition levels aim for (default 256; smaller values force more levels on
 * small inputs) and the chunk capacity, i.e. the most records bounded
 * together in LDS (default and maximum 1024; chunks of <= min(cap, 512)
 * records run one wave each, larger ones one 256-thread workgroup).  Buckets
 * over the capacity are split by further privacy-id hash bits; a bucket
 * still over it takes the global-memory path.  <= 0 keeps the current
 * value. */
int dpg_set_tuning(dpg_ctx *ctx, int32_t bucket_target, int32_t bucket_cap);

/* Contribution bounding + per-(pid,pk) accumulators + merge per partition.
 * pid, pk: device int64[n]; value: device double[n] or NULL (COUNT / PID
 * only).  out->* device arrays of out->n_partitions entries; they are
 * zero-filled by the call.  stream: hipStream_t or NULL. */
int dpg_bound_aggregate(dpg_ctx *ctx, const int64_t *pid, const int64_t *pk,
                        const double *value, int64_t n,
                        const dpg_bound_params *params, dpg_partials *out,
                        void *stream);

/* Partition selection + noise over dense partials (device arrays).
 * keep: device uint8[P]; out: device double[P * noise->n_outputs]. */
int dpg_select_and_noise(dpg_ctx *ctx, const dpg_partials *partials,
                         const dpg_select_params *select,
                         const dpg_noise_params *noise, uint8_t *keep,
                         double *out, void *stream);

/* Stream compaction of the kept partitions: writes the kept local ids to
 * kept_ids (device int64[P]) and their output rows to kept_out (device
 * double[P * n_outputs]); *n_kept (host) receives the count (synchronises
 * the stream). */
int dpg_compact_kept(dpg_ctx *ctx, const uint8_t *keep, const double *out,
                     int64_t n_partitions, int32_t n_outputs,
                     int64_t *kept_ids, double *kept_out, int64_t *n_kept,
                     void *stream);

/* The same without the host synchronisation: info (device int64[2])
 * receives the kept count (info[0]) and the bounding's error bits (info[1];
 * bit 1: the internal hash-table error dpg_compact_kept reports), in stream
 * order, so that a caller can enqueue the next release before reading them. */
int dpg_compact_kept_async(dpg_ctx *ctx, const uint8_t *keep, const double *out,
                           int64_t n_partitions, int32_t n_outputs,
                           int64_t *kept_ids, double *kept_out, int64_t *info,
                           void *stream);

/* Utility-analysis pre-aggregate: no contribution bounding; one entry per
 * distinct (privacy id, partition) pair, sorted by partition key, into
 * pairs[0, *n_pairs) (device, `capacity` entries; n always suffices), and
 * partition_start (device int64[P + 1]): the pairs of partition k are
 * [partition_start[k], partition_start[k + 1]).  Of *p only n_partitions,
 * public_mask (pairs of other partitions are dropped first), pid_min,
 * pid_count and rec_id_offset are used.  value may be NULL (sums 0).
 * n < 2^31 (else DPG_ERR_UNSUPPORTED).  *n_pairs (host) receives the pair count (synchronises the stream); if it
 * exceeds capacity the call fails with DPG_ERR_INVALID_ARG. */
int dpg_preaggregate(dpg_ctx *ctx, const int64_t *pid, const int64_t *pk, const double *value,
                     int64_t n, const dpg_bound_params *p, dpg_pair_entry *pairs,
                     int64_t capacity, int64_t *partition_start, int64_t *n_pairs,
                     void *stream);

/* Per-partition utility analysis of up to 64 configurations in one pass
 * over the sorted pre-aggregate.  Device outputs:
 *   raw    double[P][2]: privacy id count, count (RawStatistics)
 *   errors double[P][M][5][C], M = metrics present in the order SUM, COUNT,
 *          PRIVACY_ID_COUNT; the 5 fields are sum, clipping_to_min_error,
 *          clipping_to_max_error, expected_l0_bounding_error and the l0
 *          bounding variance (SumMetrics before the noise std is attached)
 *   keep   double[P][C]: partition_selection_probability_to_keep (NULL for
 *          public partitions)
 *   report double[29][F][C] or NULL: the cross-partition combine
 *          (analysis/cross_partition_combiners.py:264-343) summed per
 *          partition-size bucket (utility_analysis.py:29-39, 182-251), F =
 *          4 + 24 M fields: partitions, weight, 2 partition-info terms, then
 *          per metric its sum, 3 data-drop terms and 10 absolute + 10
 *          relative error terms, weighted by the keep probability; dividing
 *          by the weight / metric sums gives the UtilityReport
 *   *n_out (host, optional) receives the number of output partitions.
 * Partitions outside sample_mask or without pairs (and not public) stay 0
 * and are not in the output. */
int dpg_utility_analysis(dpg_ctx *ctx, const dpg_pair_entry *pairs,
                         const int64_t *partition_start, int64_t n_partitions,
                         const dpg_ua_params *params, double *raw, double *errors, double *keep,
                         double *report, int64_t *n_out, void *stream);

/* Dataset histograms over a pre-aggregate sorted by partition key (pairs,
 * partition_start as dpg_preaggregate writes them).  pre_aggregated = 0:
 * the pairs come from dpg_preaggregate, whose leader bit marks one pair per
 * privacy id (the per-privacy-id histograms count those); 1: user-supplied
 * (count, sum, n_partitions, n_contributions) rows, L0 / L1 weighted by
 * 1 / n_partitions per exact value and rounded half to even
 * (computing_histograms.py:81-102, 482-529).  All outputs are device
 * arrays, zero-filled by the call. */
int dpg_dataset_histograms(dpg_ctx *ctx, const dpg_pair_entry *pairs, int64_t n_pairs,
                           const int64_t *partition_start, int64_t n_partitions,
                           int32_t pre_aggregated, const dpg_hist_out *out, void *stream);

/* The same histograms (pre_aggregated = 0) in three phases, for several
 * ranks: between the phases the caller merges what is not a sum of per-rank
 * bins -- the per-partition totals (COUNT_PER_PARTITION and
 * PRIVACY_ID_PER_PARTITION bin a partition by its totals over all ranks) and
 * the range of the pair sums (the LINF_SUM edges).  L0, L1 and LINF bins of
 * ranks that hold disjoint privacy ids simply add (counts, sums) and max
 * (maxima).  All three calls are stream-ordered without a host
 * synchronisation, record their stages for dpg_last_stage_times ("hist.pairs",
 * "hist.partials", "hist.partitions", "hist.sums") and return
 * DPG_ERR_INVALID_ARG for null, negative or oversized arguments.  In one
 * process dpg_hist_pairs, dpg_hist_partitions on its part_rows / part_count
 * and dpg_hist_sums on its sum_range give dpg_dataset_histograms' outputs
 * (integers, edges and maxima bit for bit) and read the pairs as often: twice.
 *
 * dpg_hist_pairs: one pass over the pk-sorted pairs of dpg_preaggregate.
 * Zero-fills int_bins (device [5][DPG_HIST_INT_BINS][3]) and fills histograms
 * L0, L1 and LINF; writes part_rows[k] (pairs of partition k) and
 * part_count[k] (records), device int64[n_partitions] -- the rows / count
 * layout dpg_pack_partials reads -- and sum_range (device double[2]): the
 * smallest and largest pair sum, (+inf, -inf) when n_pairs == 0 (then pairs
 * and partition_start may be NULL). */
int dpg_hist_pairs(dpg_ctx *ctx, const dpg_pair_entry *pairs, int64_t n_pairs,
                   const int64_t *partition_start, int64_t n_partitions, uint64_t *int_bins,
                   int64_t *part_rows, int64_t *part_count, double *sum_range, void *stream);

/* Adds COUNT_PER_PARTITION (count) and PRIVACY_ID_PER_PARTITION (rows) of the
 * n partitions whose totals are given (device int64[n] each) to int_bins; a
 * partition with rows == 0 opens no bin.  Accumulates: no zero-fill. */
int dpg_hist_partitions(dpg_ctx *ctx, const int64_t *rows, const int64_t *count, int64_t n,
                        uint64_t *int_bins, void *stream);

/* LINF_SUM of this rank's pairs between the edges of sum_range (device
 * double[2]: the range of the whole dataset).  Zero-fills the four outputs
 * (as dpg_hist_out describes them); with min <= max writes lowers =
 * np.linspace(min, max, DPG_HIST_SUM_BINS + 1) -- also when n_pairs == 0, so
 * that every rank holds the same edges -- and bins the pair sums.  min > max
 * (no pair anywhere): everything stays zero.  sum_max comes out as doubles,
 * 0.0 in a bin without pairs: a caller that merges ranks takes the maximum
 * only over the bins whose sum_count is nonzero (distributed.merge_histograms
 * sends order-preserving integer keys of them, the smallest key for an empty
 * bin). */
int dpg_hist_sums(dpg_ctx *ctx, const dpg_pair_entry *pairs, int64_t n_pairs,
                  const double *sum_range, uint64_t *sum_count, double *sum_sum, double *sum_max,
                  double *lowers, void *stream);

/* The utility analysis' partition sampler (partitions_sampling_prob < 1,
 * pipeline_dp/sampling_utils.py:32-51) for integer partition keys.  Key i is
 * keys[i] (device int64[n]) or, with keys == NULL, key_lo + i * key_stride
 * (dense ids; several ranks: the owned slice).  H(key) is the big-endian
 * first 8 bytes of SHA-1 over the ASCII decimal repr of the signed key ("-"
 * for negatives, no leading zeros), i.e.
 * int(hashlib.sha1(repr(key).encode()).hexdigest()[:16], 16).  Bit i of mask
 * (bit i & 7 of byte i >> 3, the layout dpg_ua_params.sample_mask reads) is
 * set iff keep_all != 0 or H(key_i) < bound, compared as unsigned 64-bit
 * integers; keep_all stands for the bound 2^64 (round(2^64 * p) for p just
 * below 1).  mask: device, 8 * ceil(n / 64) bytes, 8-byte aligned; every bit
 * at an index >= n inside it is written as 0.  hashes (device uint64[n], or
 * NULL) receives H of every key.  Stream-ordered, no host synchronisation;
 * the stage is appended to the running list of dpg_last_stage_times as
 * "ua.sample" (closed by the mark "ua.sampled"; a call right behind another
 * replaces its entry).  A null mask, n < 0 or a misaligned pointer:
 * DPG_ERR_INVALID_ARG. */
int dpg_sample_partitions(dpg_ctx *ctx, const int64_t *keys, int64_t key_lo, int64_t key_stride,
                          int64_t n, uint64_t bound, int32_t keep_all, uint8_t *mask,
                          uint64_t *hashes, void *stream);

/* How a public-partition list relates to the data
 * (analysis/dataset_summary.py): pk (device int64[n]) holds dense ids in
 * [0, n_partitions), public_mask is the device bitmap of the public ones.
 * counts (device int64[3]) receives the number of partitions that are
 * present in pk and public, present and not public, public and not present.
 * Synchronises the stream once; a key outside [0, n_partitions):
 * DPG_ERR_KEY_RANGE. */
int dpg_partition_summary(dpg_ctx *ctx, const int64_t *pk, int64_t n, int64_t n_partitions,
                          const uint8_t *public_mask, int64_t *counts, void *stream);

/* ---- multi-GPU: an RCCL communicator for the partial merge ----
 * One process per GPU, records sharded by privacy id (bounding is then
 * shard-local).  Rank 0 calls dpg_comm_unique_id; the
 * DPG_COMM_ID_BYTES bytes reach every rank by the host's own means (MPI,
 * TCP, a shared file); each rank then attaches a communicator to its
 * context.  RCCL is loaded on first use (dlopen of librccl), so libdpg.so
 * has no link-time dependency on it and shares the copy a host such as
 * PyTorch has already loaded.  Replaces the reference's shuffle of
 * (partition key, accumulator) pairs between workers
 * (pipeline_backend.py:712-823, combine_accumulators_per_key on Beam/Spark). */
#define DPG_COMM_ID_BYTES 128
int dpg_comm_unique_id(uint8_t *id);
int dpg_ctx_create_comm(dpg_ctx *ctx, const uint8_t *id, int rank, int nranks);
/* Partition ownership is interleaved: rank r owns the partitions
 * r, r + R, r + 2R, ... (R = nranks), so hot low partition ids spread over
 * every rank; slice element i is partition lo + i * R with lo = r.
 * The merge also carries each rank's internal-error flag (a bounding whose
 * hash table overflowed, dpg_compact_kept's error): every rank receives the
 * sum of all flags and latches it, so a failure on any rank fails the
 * dpg_compact_kept of every rank instead of releasing partials of a
 * mis-bounded shard.
 *
 * dpg_reduce_scatter_partials sums the dense partials of every rank (ONE
 * ncclReduceScatter of all non-null arrays packed as float64 -- exact below
 * 2^53) and writes this rank's slice (n = number of partitions = r mod R
 * in [0, P)) into `slice` (its arrays hold >= S = ceil(P / R) entries; the
 * same arrays non-null as in `full`; slice->n_partitions is set to n).
 * Stream-ordered on `stream`. */
int dpg_reduce_scatter_partials(dpg_ctx *ctx, const dpg_partials *full, dpg_partials *slice,
                                int64_t *lo, int64_t *n, void *stream);
/* The same merge with the host's own collective (MPI, gloo, a TCP ring):
 * dpg_pack_partials writes the non-null arrays of `full` as float64 in the
 * reduce-scatter layout pack[rank][B], B = arrays * S + 1: [array][S] with
 * element i = partition i * R + rank (zero past P; array order rows, count,
 * sum, nsum, nsq), then this rank's error flag (pack holds nranks * B
 * doubles); after the host's element-wise sum over ranks delivers this
 * rank's block part[B], dpg_unpack_partials writes it into `slice` (its
 * non-null arrays name the packed ones), latches a nonzero error sum and
 * returns lo = rank and n.  Stream-ordered on `stream`. */
int dpg_pack_partials(dpg_ctx *ctx, const dpg_partials *full, int nranks, double *pack,
                      void *stream);
int dpg_unpack_partials(dpg_ctx *ctx, const double *part, int64_t n_partitions, int nranks,
                        int rank, dpg_partials *slice, int64_t *lo, int64_t *n, void *stream);
/* The error flag alone, for a merge the host routes itself (e.g. a sparse
 * all-to-all of the occupied partitions): dpg_export_error writes 1.0 to
 * device *dst if the context's last bounding latched an internal error, else
 * 0.0; dpg_import_error latches the error if any of the n device doubles at
 * src is nonzero.  Both stream-ordered, no host synchronisation. */
int dpg_export_error(dpg_ctx *ctx, double *dst, void *stream);
int dpg_import_error(dpg_ctx *ctx, const double *src, int64_t n, void *stream);

/* ---- multi-GPU: records to the rank that owns their privacy id ----
 * Bounding is shard-local only if every privacy id lives on one rank.  The
 * owner of a privacy id is shard(pid) = umulhi((uint32_t)pid * 0x9E3779B1u,
 * nranks) (distributed.shard_of).  The split below orders one rank's records
 * by owner for the host's record all-to-all; the check counts the records a
 * rank holds but does not own.  Replaces the reference's framework shuffle
 * that groups each privacy id's records before sampling
 * (contribution_bounders.py:86-92, pipeline_backend.py:264-276).
 * The split works on tiles of DPG_SHARD_TILE records (csrc/dpg_shard.h). */
#define DPG_SHARD_MAX_RANKS 64
/* Stable split of n records by owner rank d = shard(pid), nranks <= DPG_SHARD_MAX_RANKS.
 * out_*: device arrays of n entries, destination-major: the records of
 * destination d occupy [sum(counts[0..d)), +counts[d]) in their input order.
 * value / out_value may both be NULL.  counts: device int64[nranks].
 * n < 2^31 (else DPG_ERR_UNSUPPORTED); n == 0 gives all-zero counts.
 * Stream-ordered, no host synchronisation. */
int dpg_shard_records(dpg_ctx *ctx, const int64_t *pid, const int64_t *pk, const double *value,
                      int64_t n, int nranks, int64_t *out_pid, int64_t *out_pk,
                      double *out_value, int64_t *counts, void *stream);
/* *n_bad (device int64) = number of records with shard(pid) != rank.
 * Stream-ordered, no host synchronisation. */
int dpg_check_shard(dpg_ctx *ctx, const int64_t *pid, int64_t n, int nranks, int rank,
                    int64_t *n_bad, void *stream);
/* The same two calls for wide privacy ids (ColumnarData(wide_privacy_ids=True):
 * any int64): identical contracts, arguments and errors; only the owner is
 * another function, of all 64 bits of the id,
 *   shard_wide(pid) = ((fmix64(pid) >> 32) * nranks) >> 32
 * (fmix64 as given with the key dictionary below; host side:
 * distributed.shard_of_wide = distributed.key_owner).  Ids that differ only
 * above bit 31, which shard() sends to one rank, spread over all of them. */
int dpg_shard_records_wide(dpg_ctx *ctx, const int64_t *pid, const int64_t *pk,
                           const double *value, int64_t n, int nranks, int64_t *out_pid,
                           int64_t *out_pk, double *out_value, int64_t *counts, void *stream);
int dpg_check_shard_wide(dpg_ctx *ctx, const int64_t *pid, int64_t n, int nranks, int rank,
                         int64_t *n_bad, void *stream);

/* ---- multi-GPU: partition-keyed items to the rank that owns their partition ----
 * A release with percentiles or VECTOR_SUM sends its kept tree keys, or the
 * occupied partitions of its per-rank vector sums, to the partitions' owners
 * (pk mod nranks, distributed.owner_of) between the bounding and the
 * selection (distributed.exchange_owner_keys; csrc/dpg_owner.h).
 *
 * Stable split of keys[0, *n_keys) (device uint64[n_max]; *n_keys is a device int64,
 * *n_keys <= n_max < 2^31) by the owner of their partition.
 *   pk    = key >> low_bits           (pk < 2^32 - 1, 0 <= low_bits <= 32)
 *   owner = pk % nranks               (1 <= nranks <= DPG_SHARD_MAX_RANKS)
 * out_keys (device uint64[n_max]) is destination-major, in input order within
 * a destination: the keys of destination d occupy [sum(counts[0..d)), +counts[d]).
 * Each key is rewritten for its owner as
 *   (pk / nranks) << low_bits | (key & (2^low_bits - 1)).
 * out_src (device uint32[n_max], may be NULL) is the input position of every
 * output entry. counts is a device int64[nranks].
 * Entries past *n_keys are neither read nor written. *n_keys == 0 gives
 * all-zero counts (n_max == 0 too: the key pointers may then be NULL).
 * nranks or low_bits out of range, n_max < 0 or a NULL n_keys / counts:
 * DPG_ERR_INVALID_ARG; n_max >= 2^31: DPG_ERR_UNSUPPORTED; both before any
 * device work.
 * Stream-ordered, no host synchronisation. */
int dpg_owner_split_keys(dpg_ctx *ctx, const uint64_t *keys, const int64_t *n_keys,
                         int64_t n_max, int32_t low_bits, int nranks,
                         uint64_t *out_keys, uint32_t *out_src, int64_t *counts,
                         void *stream);

/* ---- sparse partition keys: a write-once hash dictionary on the device ----
 * Partition keys that are not dense ids (hashes, timestamps, product ids) get
 * global dense ids from a dictionary built over every rank's distinct keys
 * (distributed.build_key_dictionary; csrc/dpg_keydict.h).  The four calls
 * below are its device side: the distinct keys of a record column by one
 * probe per record, their compaction, and the id of every record once the
 * distinct keys have theirs.
 *
 * The table is the caller's: slots (device uint64[capacity], capacity a power
 * of two in [64, 2^31]) filled with DPG_KEYDICT_EMPTY before the first
 * insert, and slot_ids (device uint32[capacity], any content).  A slot goes
 * from DPG_KEYDICT_EMPTY to a key once and never changes again.  The key
 * INT64_MIN has the bit pattern of DPG_KEYDICT_EMPTY: it is reserved, counted
 * and never inserted.
 *   h     = fmix64(key)       murmur3's finaliser on the key's 64 bits:
 *                             k ^= k >> 33; k *= 0xff51afd7ed558ccd;
 *                             k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33
 *   home  = h & (capacity - 1), linear probing with wrap-around
 *   owner = ((h >> 32) * nranks) >> 32     (host side: distributed.key_owner)
 * Every probe sequence ends after at most `capacity` steps.
 *
 * All four: n < 2^31 (else DPG_ERR_UNSUPPORTED); n == 0 is a no-op (the
 * per-record pointers may then be NULL); a bad capacity, n < 0 or a NULL
 * pointer: DPG_ERR_INVALID_ARG; both before any device work.  The counters
 * are added to, so the caller zeroes them.  Stream-ordered, no host
 * synchronisation. */
#define DPG_KEYDICT_EMPTY 0x8000000000000000ull
/* Inserts the distinct values of keys[0, n).  info (device int64[2]):
 * info[0] += records holding the reserved key, info[1] += records that found
 * no slot (the table is full: with capacity >= 2 x the distinct keys this
 * stays 0).  May be called several times on one table. */
int dpg_keydict_insert(dpg_ctx *ctx, const int64_t *keys, int64_t n, uint64_t *slots,
                       int64_t capacity, int64_t *info, void *stream);
/* out_keys (device int64[capacity]) receives the keys of the occupied slots,
 * in no particular order, *n_keys (device int64) their number. */
int dpg_keydict_keys(dpg_ctx *ctx, const uint64_t *slots, int64_t capacity, int64_t *out_keys,
                     int64_t *n_keys, void *stream);
/* slot_ids[slot of keys[i]] = ids[i] for i < n (ids: device int64, every value
 * in [0, 2^32 - 1); equal keys must carry equal ids).  *n_missing (device
 * int64) += the keys that are not in the table, the reserved key included. */
int dpg_keydict_assign(dpg_ctx *ctx, const int64_t *keys, const int64_t *ids, int64_t n,
                       const uint64_t *slots, uint32_t *slot_ids, int64_t capacity,
                       int64_t *n_missing, void *stream);
/* out_ids[i] (device int64[n]) = the id assigned to keys[i]; a key that is
 * absent or reserved gives -1 and *n_missing (device int64) += 1.  The id of
 * a key that is present but was never assigned is unspecified. */
int dpg_keydict_lookup(dpg_ctx *ctx, const int64_t *keys, int64_t n, const uint64_t *slots,
                       const uint32_t *slot_ids, int64_t capacity, int64_t *out_ids,
                       int64_t *n_missing, void *stream);
/* Insert once, never probe again (wide privacy ids:
 * distributed.encode_privacy_ids).  The table is write-once and a key never
 * moves, so the slot a record finds when it is inserted is final.  The two
 * calls below follow the contract of the four above.
 *
 * dpg_keydict_insert with the same protocol and the same info counters, which
 * also stores every record's final slot: out_slots[i] (device uint32[n]) is
 * the slot that holds keys[i], or 0xFFFFFFFF (never a slot: capacity <= 2^31)
 * for a record that holds the reserved key or found no slot.  May be called
 * several times on one table. */
int dpg_keydict_insert_slots(dpg_ctx *ctx, const int64_t *keys, int64_t n, uint64_t *slots,
                             int64_t capacity, uint32_t *out_slots, int64_t *info, void *stream);
/* out_ids[i] (device int64[n]) = slot_ids[out_slots[i]] for i < n; an entry
 * that is not a slot of the table (0xFFFFFFFF) gives -1 and *n_missing (device
 * int64) += 1.  Reads neither the keys nor the slots: 4 bytes in, 8 bytes out
 * and one 4-byte gather per record. */
int dpg_keydict_gather_ids(dpg_ctx *ctx, const uint32_t *out_slots, int64_t n,
                           const uint32_t *slot_ids, int64_t capacity, int64_t *out_ids,
                           int64_t *n_missing, void *stream);

/* ---- string columns: bytes to 64-bit keys, checked for collisions ----
 * A string column (pipelinedp_amd.StringColumn) is Arrow's variable-width
 * layout: offsets (device int64[n + 1]) and data (device uint8[data_len]);
 * record i is the bytes data[offsets[i], offsets[i + 1]).  The three calls
 * below reduce it to what the table calls above take (csrc/dpg_strkey.h;
 * DESIGN.md section 18): a 64-bit key per record, the first record of every
 * slot, and the count of records whose bytes differ from that record's -- so
 * a hash collision is found, never released as one merged partition.
 *
 * All three follow the table calls' contract: n < 2^31 (else
 * DPG_ERR_UNSUPPORTED); n == 0 is a no-op (the per-record pointers may then be
 * NULL); n < 0, data_len < 0, a bad capacity or a NULL pointer (data may be
 * NULL when data_len == 0): DPG_ERR_INVALID_ARG; both before any device work.
 * The counters are added to, so the caller zeroes them.  Stream-ordered, no
 * host synchronisation.
 *
 * The key of a string s of len bytes under a 64-bit seed, with fmix64 as
 * given with the key dictionary above and all arithmetic modulo 2^64:
 *   h = fmix64(seed ^ (len * 0x9E3779B97F4A7C15))
 *   for k = 0 .. ceil(len / 8) - 1:
 *       w = the bytes s[8k .. 8k + 8) as a little-endian 64-bit word, bytes
 *           at positions >= len taken as zero
 *       h = fmix64(h ^ w)
 *   key = h, except that h == DPG_KEYDICT_EMPTY gives DPG_KEYDICT_EMPTY ^ 1:
 *   the table's reserved key never comes out.
 * The empty string has no words: its key is fmix64(seed).
 *
 * out_keys[i] (device int64[n]) = the key of record i.  A record whose
 * offsets are not 0 <= offsets[i] <= offsets[i + 1] <= data_len reads nothing,
 * gets the key 0 and adds 1 to info[0] (device int64[1]).  No byte outside
 * data[0, data_len) is read, whatever the alignment of data and of the
 * strings in it. */
int dpg_string_hash(dpg_ctx *ctx, const int64_t *offsets, const uint8_t *data, int64_t data_len,
                    int64_t n, uint64_t seed, int64_t *out_keys, int64_t *info, void *stream);
/* rep (device uint32[capacity], capacity as for the table, filled with
 * 0xFFFFFFFF by the caller): afterwards rep[s] is the smallest i < n with
 * rec_slots[i] == s (rec_slots: device uint32[n], as dpg_keydict_insert_slots
 * wrote it), and still 0xFFFFFFFF for a slot no record has.  Entries of
 * rec_slots that are not a slot of the table (0xFFFFFFFF) are skipped.  May be
 * called several times on one rep: values only fall. */
int dpg_keydict_representatives(dpg_ctx *ctx, const uint32_t *rec_slots, int64_t n,
                                int64_t capacity, uint32_t *rep, void *stream);
/* *n_mismatch (device int64) += the records i < n whose bytes differ from
 * the bytes of record rep[rec_slots[i]]: length first, then content.  Records
 * with rec_slots[i] == 0xFFFFFFFF are skipped; every other entry must be a
 * slot of the table rep belongs to.  Offsets are checked as in
 * dpg_string_hash: a record with invalid offsets -- its own or its
 * representative's -- or whose slot has no representative below n counts as a
 * mismatch and reads nothing. */
int dpg_string_verify(dpg_ctx *ctx, const int64_t *offsets, const uint8_t *data, int64_t data_len,
                      int64_t n, const uint32_t *rec_slots, const uint32_t *rep,
                      int64_t *n_mismatch, void *stream);

/* ---- string columns: gathered into a packed column, runs of equal keys ----
 * What the global string dictionary (distributed.build_string_dictionary;
 * csrc/dpg_strpack.h) needs beyond the calls above:
 * chosen records of a column packed back to back -- the lengths, a prefix sum
 * by the caller, the bytes -- and, at the owner of a key, the check that every
 * run of equal keys holds one string.
 *
 * All three follow the contract of the string calls above: every count < 2^31
 * (else DPG_ERR_UNSUPPORTED); m == 0 is a no-op (the per-element pointers may
 * then be NULL); a negative count or a NULL pointer (data may be NULL when
 * data_len == 0, out_data when out_total == 0): DPG_ERR_INVALID_ARG; both
 * before any device work.  The counters are added to, so the caller zeroes
 * them.  Stream-ordered, no host synchronisation.  The column is offsets
 * (device int64[n + 1]) and data (device uint8[data_len]) as above; records
 * (device int64[m]) may repeat and come in any order.
 *
 * out_len[j] (device int64[m]) = the byte length of record records[j].  A
 * records[j] outside [0, n), or offsets that are not 0 <= offsets[r] <=
 * offsets[r + 1] <= data_len, gives length 0 and adds 1 to info[0] (device
 * int64[1]). */
int dpg_string_lengths(dpg_ctx *ctx, const int64_t *offsets, int64_t data_len, int64_t n,
                       const int64_t *records, int64_t m, int64_t *out_len, int64_t *info,
                       void *stream);
/* out_data[out_offsets[j], out_offsets[j + 1]) (out_offsets: device
 * int64[m + 1]; out_data: device uint8[out_total], not overlapping data)
 * receives the bytes of record records[j].  A j whose record or offsets are
 * invalid as above, whose out range is not 0 <= out_offsets[j] <=
 * out_offsets[j + 1] <= out_total, or whose out range is not as long as the
 * record writes nothing and adds 1 to info[0] (device int64[1]).  No byte
 * outside data[0, data_len) is read and none outside the j's own out range is
 * written, whatever the alignment of data and of out_data. */
int dpg_string_pack(dpg_ctx *ctx, const int64_t *offsets, const uint8_t *data, int64_t data_len,
                    int64_t n, const int64_t *records, int64_t m, const int64_t *out_offsets,
                    uint8_t *out_data, int64_t out_total, int64_t *info, void *stream);
/* keys (device int64[m]) with equal keys adjacent; order (device uint32[m], or
 * NULL = the identity): entry j stands for string order[j] of a column of
 * n_strings strings.  head[j] (device uint8[m]) = 1 if j == 0 or keys[j] !=
 * keys[j - 1], else 0.  An entry with head[j] == 0 is compared with the entry
 * before it, string order[j] with string order[j - 1], length first and then
 * content: a difference adds 1 to info[0] (device int64[2]).  An index outside
 * [0, n_strings) or invalid offsets on either side read nothing, count as a
 * difference (info[0] += 1) and add 1 to info[1].  With info[0] == 0 every run
 * of equal keys holds byte-equal strings. */
int dpg_string_verify_runs(dpg_ctx *ctx, const int64_t *keys, const uint32_t *order,
                           const int64_t *offsets, const uint8_t *data, int64_t data_len,
                           int64_t n_strings, int64_t m, uint8_t *head, int64_t *info,
                           void *stream);

/* ---- multi-GPU utility analysis: pairs to the rank that owns their partition ----
 * The per-partition utility combiners need every (privacy id, partition) pair
 * of a partition on one rank, so each rank's pre-aggregate travels to the
 * partitions' owners between dpg_preaggregate and dpg_utility_analysis
 * (distributed.exchange_owner_pairs; csrc/dpg_pairx.h).
 *
 * Stable split of pairs[0, n) (device; n is a host count, as dpg_preaggregate
 * returned it) by owner = pk % nranks (1 <= nranks <= DPG_SHARD_MAX_RANKS).
 * out_pairs (device, n entries, not overlapping pairs) is destination-major,
 * in input order within a destination: the pairs of destination d occupy
 * [sum(counts[0..d)), +counts[d]).  Every entry's pk is rewritten to
 * pk / nranks; its other 20 bytes -- the leader bit and the bits of sum
 * included -- are carried unchanged.  counts is a device int64[nranks].
 * n == 0 gives all-zero counts (the pair pointers may then be NULL).  nranks
 * out of range, n < 0, a NULL counts or (n > 0) pairs / out_pairs:
 * DPG_ERR_INVALID_ARG; n >= 2^31: DPG_ERR_UNSUPPORTED; both before any device
 * work.  Stream-ordered, no host synchronisation. */
int dpg_owner_split_pairs(dpg_ctx *ctx, const dpg_pair_entry *pairs, int64_t n, int nranks,
                          dpg_pair_entry *out_pairs, int64_t *counts, void *stream);

/* Merge of pk-sorted runs into one pre-aggregate.  pairs (device) holds nruns
 * consecutive runs (1 <= nruns <= DPG_SHARD_MAX_RANKS); run r is
 * [run_start[r], run_start[r + 1]) (host int64[nruns + 1], run_start[0] = 0,
 * ascending, n = run_start[nruns] < 2^31), each ascending by pk.  out_pairs
 * (device, n entries, not overlapping pairs) receives them ascending by pk
 * and, within a partition, by run and then by position in the run: a fixed
 * order, the same on every execution.  partition_start (device
 * int64[n_partitions + 1]) is written as dpg_preaggregate writes it.  A
 * counting placement, not a sort: O(n + nruns * n_partitions) work, integer
 * only; nruns * n_partitions < 2^32 - 1 (else DPG_ERR_UNSUPPORTED, as n >=
 * 2^31).
 * *n_bad (device int64) counts the entries with pk >= n_partitions or with a
 * pk below that of an in-range predecessor in their run.  They are never
 * written.  *n_bad == 0 if and only if every run is in range and ascending.
 * The other entries are placed as if the bad ones were absent when every bad
 * entry sits between entries of two different partitions (or at an end of its
 * run) and the runs without the bad entries are ascending; otherwise their
 * places, always inside out_pairs, are unspecified and slots may stay
 * unwritten.  Whatever the input, partition_start is ascending and
 * partition_start[n_partitions] <= n, so a reader of the result stays inside
 * out_pairs.
 * Empty runs, n == 0 (the pair pointers may then be NULL) and nruns == 1 (a
 * copy and the starts) are valid.  Bad arguments: DPG_ERR_INVALID_ARG before
 * any device work.  Stream-ordered, no host synchronisation. */
int dpg_merge_pair_runs(dpg_ctx *ctx, const dpg_pair_entry *pairs, const int64_t *run_start,
                        int nruns, int64_t n_partitions, dpg_pair_entry *out_pairs,
                        int64_t *partition_start, int64_t *n_bad, void *stream);

/* ---- percentiles: kept records, quantile tree (combiners.py:532-611) ----
 * Stable LSD radix sort of n (key, payload) pairs by the key bits
 * [begin_bit, end_bit) (0 <= begin_bit <= end_bit <= 64), 8 bits per pass;
 * a pass whose digit takes one value over the whole input is skipped on the
 * device.  Device arrays of n entries; vals_in / vals_out may both be NULL
 * (keys only).  The outputs must not overlap the inputs.  n < 2^31 (else
 * DPG_ERR_UNSUPPORTED); n == 0 is a no-op.  Stream-ordered, no host
 * synchronisation (csrc/dpg_rsort.h). */
int dpg_sort_pairs_u64(dpg_ctx *ctx, const uint64_t *keys_in, const uint32_t *vals_in, int64_t n,
                       int32_t begin_bit, int32_t end_bit, uint64_t *keys_out, uint32_t *vals_out,
                       void *stream);

/* keep[i] (device uint8[n]) = 1 iff record i is in the kept set of
 * dpg_bound_aggregate under the same context seed and params (nonce,
 * rec_id_offset, public_mask, pid_min / pid_count, mode, mpc, mcpp): pairs of
 * a privacy id ascending by (pair priority << 32 | pk), the first mpc kept;
 * records of a pair ascending by the 64-bit record priority, the first mcpp
 * kept (DPG_MODE_CROSS_PARTITION: all of them).  DPG_MODE_PER_PRIVACY_ID is
 * DPG_ERR_UNSUPPORTED, as is n >= 2^31.  A privacy id outside a declared
 * range or a pk outside [0, P) is never kept and sets bit 0 of the
 * context's device error word, which dpg_compact_kept_async copies to
 * info[1] (the call itself cannot report it: it does not wait for the
 * device).  pid_count == 0 needs no range reduction here: ids are compared
 * as 64-bit values.  Stream-ordered, no host synchronisation
 * (csrc/dpg_records.h). */
int dpg_bound_records(dpg_ctx *ctx, const int64_t *pid, const int64_t *pk, int64_t n,
                      const dpg_bound_params *params, uint8_t *keep, void *stream);

typedef struct dpg_quantile_params {
    double lo, hi;        /* the tree covers [lo, hi]: min_value, max_value  */
    int32_t noise_kind;   /* DPG_NOISE_*                                     */
    int32_t n_quantiles;  /* 1..16                                           */
    double scale;         /* b or sigma of every node count                  */
    double quantiles[16]; /* in [0, 1]                                       */
    int64_t pk_offset;    /* global pk of local partition i is               */
    int64_t pk_stride;    /*   pk_offset + i * pk_stride; <= 0 means 1       */
    uint64_t nonce;       /* per-release nonce (see dpg_bound_params)        */
} dpg_quantile_params;

/* Tree keys: keys[0, *n_keys) (device uint64[n], device int64) receive
 * pk << 16 | leaf of every record with keep[i] != 0 and a non-NaN value,
 * sorted; leaf = min(65535, floor((clamp(v, lo, hi) - lo) * 65536 / (hi - lo)))
 * (0 when lo == hi).  pk in [0, P), P < 2^32 - 1; n < 2^31.  Stream-ordered,
 * no host synchronisation. */
int dpg_quantile_keys(dpg_ctx *ctx, const int64_t *pk, const double *value, const uint8_t *keep,
                      int64_t n, int64_t n_partitions, const dpg_quantile_params *qparams,
                      uint64_t *keys, int64_t *n_keys, void *stream);

/* out[k][j] (device double[P][n_quantiles]) = the quantiles[j]-quantile of
 * partition k from its noised 16-ary tree of height 4 (Google's walk:
 * children below 0.0075 of their siblings' clamped total are dropped, the
 * first child whose inclusive share reaches rank - 1e-6 is entered, the
 * result interpolates over the last node's range).  The noised count of
 * node nu is add_noise(kind, count, scale, stream seed, global pk,
 * DPG_SLOT_QNODE0 + nu): a pure function of (seed, nonce, partition, node).
 * Rows of partitions with keep_partition[k] == 0 (device uint8[P], or NULL:
 * all) are left untouched.  keys / n_keys as dpg_quantile_keys wrote them
 * (csrc/dpg_quantile.h). */
int dpg_quantiles(dpg_ctx *ctx, const uint64_t *keys, const int64_t *n_keys, int64_t n_partitions,
                  const dpg_quantile_params *qparams, const uint8_t *keep_partition, double *out,
                  void *stream);

/* ---- VECTOR_SUM: per-partition vector sums over the kept records ---- */
#define DPG_NORM_LINF 0
#define DPG_NORM_L1 1
#define DPG_NORM_L2 2
#define DPG_VECTOR_MAX_SIZE 4096
#define DPG_VSUM_CHUNK 512 /* sorted rows summed by one wave */

/* The inverted index of the kept records: keys[0, *n_keys) (device uint64[n],
 * device int64) receive pk << 31 | i of every record i with keep[i] != 0 and
 * pk in [0, P), ascending: the records of a partition are consecutive, in
 * input order.  n < 2^31 (else DPG_ERR_UNSUPPORTED), P < 2^32 - 1; n == 0
 * gives *n_keys = 0.  Stream-ordered, no host synchronisation. */
int dpg_vector_index(dpg_ctx *ctx, const int64_t *pk, const uint8_t *keep, int64_t n,
                     int64_t n_partitions, uint64_t *keys, int64_t *n_keys, void *stream);

/* out[k][d] (device double[P][D], zero-filled by the call) = the sum of
 * value[i][d] (device double[n][D], row-major) over the keys of partition k.
 * No atomics: the order of the additions is a fixed function of the sorted
 * keys and D (csrc/dpg_vsum.h states it), so two calls agree bit for bit on
 * any grid.  keys / n_keys as dpg_vector_index wrote them.  1 <= D <=
 * DPG_VECTOR_MAX_SIZE (larger: DPG_ERR_UNSUPPORTED, as n >= 2^31).
 * Stream-ordered, no host synchronisation. */
int dpg_vector_sums(dpg_ctx *ctx, const uint64_t *keys, const int64_t *n_keys, const double *value,
                    int64_t n, int32_t size, int64_t n_partitions, double *out, void *stream);

typedef struct dpg_vector_params {
    int32_t size;       /* D = vector_size                                   */
    int32_t norm_kind;  /* DPG_NORM_*                                        */
    double max_norm;    /* vector_max_norm                                   */
    int32_t noise_kind; /* DPG_NOISE_*                                       */
    int32_t reserved;
    double scale;       /* b or sigma of every coordinate                    */
    int64_t pk_offset;  /* global pk of local partition i is                 */
    int64_t pk_stride;  /*   pk_offset + i * pk_stride; <= 0 means 1         */
    uint64_t nonce;     /* per-release nonce (see dpg_bound_params)          */
} dpg_vector_params;

/* out[k][d] = add_noise(kind, clip(sums[k])[d], scale, stream seed,
 * pk_offset + k * pk_stride, DPG_SLOT_VEC0 + d) for the rows (device
 * double[P][D]) with keep_partition[k] != 0 (device uint8[P], or NULL: all);
 * the other rows of out are left untouched.  clip: DPG_NORM_LINF clamps
 * every coordinate to [-max_norm, max_norm]; DPG_NORM_L1 / L2 scale the row
 * by min(1, max_norm / norm), 1 for a zero row.  out may be sums.
 * Stream-ordered, no host synchronisation. */
int dpg_vector_clip_noise(dpg_ctx *ctx, const double *sums, int64_t n_partitions,
                          const dpg_vector_params *vparams, const uint8_t *keep_partition,
                          double *out, void *stream);

/* Timing/profiling aid: per-stage device time (ms) of the last
 * dpg_bound_aggregate / dpg_preaggregate / dpg_dataset_histograms /
 * dpg_bound_records / dpg_quantile_keys / dpg_vector_index / dpg_vector_sums
 * / dpg_owner_split_keys / dpg_owner_split_pairs / dpg_merge_pair_runs call
 * ("vector:keys", "vector:sort:...", "vector:sum", "vector:merge";
 * "owner:count", "owner:scan", "owner:scatter"; "pairs:count", "pairs:scan",
 * "pairs:owner_split" (the split's scatter kernel); "pairs:bounds",
 * "pairs:scan", "pairs:merge" (the merge's placement kernel)),
 * measured with HIP events on its stream (waits for the last event).
 * names (comma separated, <= names_len bytes): e.g. "begin",
 * "partition1:hist", "partition1:scatter", "partition2:hist",
 * "partition2:scatter", "chunks", "bound.kernel=sort" (zero-length marker
 * of the small-chunk kernel that ran), "bound", "bound.wide" (sort kernel:
 * chunks of more than 256 candidates), "bound.medium", "bound.tail",
 * "items:hist", "items:scatter", "reduce".  With DPG_DEBUG_ITEM_PATHS set
 * in the environment (a test hook: one more host synchronisation) the
 * zero-length markers "items.regions=window" / "items.regions=lookup" follow
 * "items:scatter": sub-tiles of the first item level whose regions were
 * resolved wave-uniformly / by the per-lane lookup.  With
 * DPG_DEBUG_TEAM_PATHS set (the same kind of hook) the markers
 * "team.pieces=pair" / "team.pieces=lookup" follow "partition2:team" when
 * level 2 runs by teams on level-1 pieces: members' shares loaded with one
 * compare per load / by the 8-piece lookup. */
int dpg_last_stage_times(dpg_ctx *ctx, char *names, size_t names_len,
                         double *ms, int32_t max_stages, int32_t *n_stages);

#ifdef __cplusplus
}
#endif
#endif /* DPG_H_ */
