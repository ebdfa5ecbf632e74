"""Exact values for bit-exact parity tests, the bounding modes of the mode
matrix and its seeded inputs (shared by tests/test_exact_values_cpu.py, which
checks on the CPU that every case's bounds bind, and
tests/test_gpu_mode_matrix.py).

Values are k / 4096 with k an integer in [-2 * 4096, 12 * 4096); every
clipping bound used with them is a multiple of 1/4096, and so is the midpoint
of every value range ([-1, 5] -> 2, [0, 10] -> 5).  Each term x, x - mid and
(x - mid)^2 is then a multiple of 2^-24 below 2^6, so any sum of up to 2^23
such terms is exact in float64 in any order: LDS atomics, global atomics, the
merge and the oracle's loop must all give the same bits, and the tests compare
sums with np.array_equal.  Inputs stay within 2^21 records.
"""
import functools

import numpy as np

import pipelinedp_amd as pdp
from pipelinedp_amd import combiners

FRAC_BITS = 12
SCALE = 1 << FRAC_BITS
V_LO, V_HI = -2, 12
MAX_RECORDS = 1 << 21
SEED = 0x5EED
NONCE = 0x0DDC0FFEE   # fixed release nonce: the CPU conditions hold for the very GPU runs


def exact_values(rng, n):
    """n float64 values k / 4096, k uniform in [-2 * 4096, 12 * 4096)."""
    return rng.integers(V_LO * SCALE, V_HI * SCALE, n).astype(np.float64) / SCALE


def to_fixed(x):
    """The int64 k of exact values (or bounds) k / 4096; raises if x has
    more than 12 fraction bits."""
    x = np.asarray(x, np.float64)
    k = np.rint(x * SCALE).astype(np.int64)
    if not np.array_equal(k.astype(np.float64) / SCALE, x):
        raise ValueError("value with more than 12 fraction bits")
    return k


# --------------------------------------------------------------------- modes
M = pdp.Metrics
CROSS_AND_PER, PER_PID, CROSS = (combiners.MODE_CROSS_AND_PER, combiners.MODE_PER_PID,
                                 combiners.MODE_CROSS)
NONE, CLIP_VALUE, CLIP_PARTITION = (combiners.SUM_NONE, combiners.SUM_CLIP_VALUE,
                                    combiners.SUM_CLIP_PARTITION)

# id -> (AggregateParams keywords without the contribution bounds, expected
# bounding mode, expected sum mode)
MODES = {
    "cap_sum_pp": (dict(metrics=[M.COUNT, M.SUM], min_sum_per_partition=-1.0,
                        max_sum_per_partition=9.0), CROSS_AND_PER, CLIP_PARTITION),
    "cross_sum_pp": (dict(metrics=[M.SUM, M.PRIVACY_ID_COUNT], min_sum_per_partition=-1.0,
                          max_sum_per_partition=20.0), CROSS, CLIP_PARTITION),
    "cross_rows": (dict(metrics=[M.PRIVACY_ID_COUNT]), CROSS, NONE),
    "perpid_sum_pp": (dict(metrics=[M.COUNT, M.SUM], min_sum_per_partition=-1.0,
                           max_sum_per_partition=9.0), PER_PID, CLIP_PARTITION),
    # VARIANCE is rejected with max_contributions (dp_engine.py
    # _check_aggregate_params, as the reference's); MEAN runs the same ItemV
    # items with both normalised moments
    "perpid_var": (dict(metrics=[M.MEAN, M.COUNT], min_value=-1.0, max_value=5.0),
                   PER_PID, CLIP_VALUE),
    "item32": (dict(metrics=[M.MEAN, M.SUM, M.PRIVACY_ID_COUNT], min_value=0.0, max_value=10.0),
               CROSS_AND_PER, CLIP_VALUE),
    "mean_var": (dict(metrics=[M.MEAN, M.VARIANCE, M.COUNT], min_value=-1.0, max_value=5.0),
                 CROSS_AND_PER, CLIP_VALUE),
}
CROSS_MODES = ("cap_sum_pp", "cross_sum_pp", "cross_rows", "item32")


def is_per_pid(mode):
    return MODES[mode][1] == PER_PID


# -------------------------------------------------------------------- inputs
def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _dataset(seed, n, n_pid, P, zipf):
    rng = np.random.default_rng(seed)
    pid = rng.integers(0, n_pid, n).astype(np.int64)
    pk = ((rng.zipf(zipf, n) - 1) % P).astype(np.int64)
    return pid, pk, exact_values(rng, n), P


def _wide_medium():
    rng = np.random.default_rng(77)
    P = 2000
    pid = np.concatenate([np.repeat(np.arange(6000), 200), np.repeat(np.arange(6000, 6300), 700)])
    pid = rng.permutation(pid).astype(np.int64)
    pk = ((rng.zipf(1.1, pid.size) - 1) % P).astype(np.int64)
    return pid, pk, exact_values(rng, pid.size), P


def _streamed(size):
    rng = np.random.default_rng(size)
    P = 20_000
    n_pid = 1500
    pid = np.repeat(np.arange(n_pid), size)
    pk = ((rng.zipf(1.1, pid.size) - 1) % P).astype(np.int64)
    few = np.isin(pid, np.arange(0, n_pid, 10))
    pk[few] = rng.integers(0, 3, int(few.sum())) * 7
    perm = rng.permutation(pid.size)
    pid, pk = pid[perm].astype(np.int64), pk[perm]
    return pid, pk, exact_values(rng, pid.size), P


def _oversize():
    rng = np.random.default_rng(404)
    P = 3000
    pid = rng.integers(0, 2000, 200_000)
    pk = ((rng.zipf(1.1, pid.size) - 1) % P).astype(np.int64)
    few = pid % 10 == 3
    pk[few] = rng.integers(0, 3, int(few.sum())) * 11
    return pid.astype(np.int64), pk, exact_values(rng, pid.size), P


def _wide_records():
    rng = np.random.default_rng(77)
    n, P = 300_000, 40_000_000
    ids = rng.choice(np.int64(2) ** 31, 20_000, replace=False)
    pid = ids[rng.integers(0, ids.size, n)]
    pk = rng.integers(0, P, n).astype(np.int64)
    pk[: n // 2] = (rng.zipf(1.3, n // 2) - 1) % 5000
    return pid.astype(np.int64), pk, exact_values(rng, n), P


MERGE_P = 6_000_000
MERGE_RANGE = 4096    # partitions per range of the merge (dpg_select.h kRange)
MERGE_TILE = 65536    # kept pairs per merge tile (dpg_api.hip bound_and_reduce)


def _merge_uniform():
    """Uniform keys over 6e6 partitions: ~50 kept pairs per range, so every
    range is one tile (the merge's plain-store branch)."""
    rng = np.random.default_rng(31)
    n = 300_000
    pid = rng.integers(0, 20_000, n).astype(np.int64)
    pk = rng.integers(0, MERGE_P, n).astype(np.int64)
    return pid, pk, exact_values(rng, n), MERGE_P


def _merge_hot():
    """Every key a Zipf-hot id below 4096: all kept pairs (> 65536) fall into
    range 0, which then spans several tiles (the merge's atomic branch)."""
    rng = np.random.default_rng(32)
    n = 300_000
    pid = rng.integers(0, 100_000, n).astype(np.int64)
    pk = ((rng.zipf(1.2, n) - 1) % MERGE_RANGE).astype(np.int64)
    return pid, pk, exact_values(rng, n), MERGE_P


_GENERATORS = {
    "small": lambda: _dataset(41, 400_000, 10_000, 3000, 1.1),      # ~40 records / id
    "wide_medium": _wide_medium,                                    # 200- and 700-record ids
    "streamed600": lambda: _streamed(600),
    "streamed1000": lambda: _streamed(1000),
    "oversize": _oversize,                                          # ~100 records / id
    "global": lambda: _dataset(31, 200_000, 2_000, 3000, 1.1),      # ~100 records / id
    "levels": lambda: _dataset(21, 250_000, 2_500, 5000, 1.1),      # ~100 records / id
    "wide_records": _wide_records,
    "merge_uniform": _merge_uniform,
    "merge_hot": _merge_hot,
}


@functools.lru_cache(maxsize=None)
def dataset(gen):
    """(pid, pk, value, P) of a named input; cached and read-only."""
    pid, pk, val, P = _GENERATORS[gen]()
    assert pid.size <= MAX_RECORDS
    return _freeze(pid, pk, val) + (P,)


# Contribution bounds per input: (mpc, mcpp, L).  mpc follows the source tests of
# tests/test_gpu_parity.py; mcpp is 2 (1 for mean_var, as in its MODES); L cuts
# every privacy id of the input (40 to 1000 records each).
_BOUNDS = {
    "small": (3, 2, 10),
    "wide_medium": (100, 2, 50),
    "streamed600": (8, 2, 5),
    "streamed1000": (8, 2, 5),
    "oversize": (4, 2, 5),
    "global": (3, 2, 20),
    "levels": (8, 2, 20),
    "wide_records": (3, 2, 5),
    "merge_uniform": (4, 2, 5),
    "merge_hot": (2, 2, 2),
}

# Sum bounds other than the mode's own, where those would not bind (the
# conditions of tests/test_exact_values_cpu.py decide, not the kernels):
# pairs of the merge inputs and of the 12-byte-record input are mostly single
# records, whose sum never reaches 20.
_SUM_BOUNDS = {
    ("cross_sum_pp", "merge_uniform"): (-1.0, 9.0),
    ("cross_sum_pp", "merge_hot"): (-1.0, 9.0),
    ("cross_sum_pp", "wide_records"): (-1.0, 9.0),
}

# The (mode, input) pairs of the GPU matrix.
PAIRS = (
    [(m, "small") for m in CROSS_MODES + ("perpid_sum_pp", "perpid_var")]
    + [(m, "wide_medium") for m in CROSS_MODES + ("perpid_sum_pp", "perpid_var")]
    + [(m, g) for g in ("streamed600", "streamed1000", "oversize") for m in CROSS_MODES]
    + [(m, "global") for m in ("cap_sum_pp", "cross_sum_pp", "cross_rows", "perpid_sum_pp",
                               "perpid_var")]
    + [(m, "levels") for m in ("cap_sum_pp", "cross_sum_pp", "perpid_var", "mean_var")]
    + [(m, "wide_records") for m in ("cap_sum_pp", "cross_sum_pp", "mean_var")]
    + [(m, g) for g in ("merge_uniform", "merge_hot")
       for m in ("item32", "mean_var", "cross_sum_pp")]
)


def params_kwargs(mode, gen):
    """AggregateParams keywords of a (mode, input) pair."""
    kw = dict(MODES[mode][0])
    mpc, mcpp, L = _BOUNDS[gen]
    if is_per_pid(mode):
        kw["max_contributions"] = L
    else:
        kw["max_partitions_contributed"] = mpc
        kw["max_contributions_per_partition"] = 1 if mode == "mean_var" else mcpp
    if (mode, gen) in _SUM_BOUNDS:
        kw["min_sum_per_partition"], kw["max_sum_per_partition"] = _SUM_BOUNDS[(mode, gen)]
    return kw


def make_params(mode, gen):
    """The AggregateParams a pair's release is requested with.

    Two cells are not reachable through AggregateParams and are reached
    below it, by override_plan() on the release's plan (the C ABI of
    include/dpg.h takes both):

    * perpid_sum_pp: PER_PRIVACY_ID with per-partition sum bounds is accepted
      by AggregateParams but rejected when the plan computes the SUM
      sensitivities (linf without l0: Sensitivities raises, as the
      reference's does), so the request is cap_sum_pp's.
    * item32: a plan with MEAN or VARIANCE never sets the SUM bit of the
      metric mask (the released sum comes from the normalised sum), so MEAN +
      SUM runs 24-byte ItemV items; the 32-byte Item32 layout needs that bit.
    """
    kw = params_kwargs("cap_sum_pp" if mode == "perpid_sum_pp" else mode, gen)
    if mode == "perpid_sum_pp":
        kw.update({k: MODES[mode][0][k] for k in ("min_sum_per_partition",
                                                  "max_sum_per_partition")})
    return pdp.AggregateParams(**kw)


def override_plan(plan, mode, gen):
    """Switches the plan of make_params(mode, gen) to the pair's cell where
    AggregateParams cannot (see make_params)."""
    if mode == "item32":
        plan.mask |= combiners.M_SUM      # bound fields' metric_mask and the sum partial
    if mode == "perpid_sum_pp":
        L = _BOUNDS[gen][2]
        inner = plan.bound_fields
        plan.bound_fields = lambda P: dict(inner(P), mode=PER_PID, max_contributions=L,
                                           max_partitions_contributed=0,
                                           max_contributions_per_partition=0)


def bound_fields(mode, gen):
    """The dpg_bound_params fields of a pair as the engine fills them on one
    device, with the fixed nonce."""
    P = dataset(gen)[3]
    plan = combiners.CompoundPlan(make_params(mode, gen), pdp.NaiveBudgetAccountant(1.0, 1e-6))
    override_plan(plan, mode, gen)
    return dict(plan.bound_fields(P), nonce=NONCE)
