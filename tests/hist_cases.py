"""Shared by the multi-rank histogram tests (test_gpu_hist_phases.py,
test_gpu_hist_ranks.py, test_hist_exchange_cpu.py): the dataset, the numpy
restatement of distributed.shard_of, and DatasetHistograms / raw bin arrays as
plain lists in the oracle's form (oracle/hist_oracle.py)."""
import functools

import numpy as np

N, N_PID, P_DATA, P_ALL = 80_000, 2_500, 1_290, 1_301
PID_WIDE, PID_DEEP = 2_505, 2_506  # L0 = 1100; LINF = L1 = 1200
PLANT_CANDIDATES = range(2_507, 2_600)


def shard_np(pid, world):
    """numpy restatement of distributed.shard_of (uint32 form)."""
    h = (np.asarray(pid).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


def planted_pid():
    """A privacy id whose shard differs from PID_DEEP's for 2 and for 3 ranks."""
    for p in PLANT_CANDIDATES:
        if all(shard_np([p], w)[0] != shard_np([PID_DEEP], w)[0] for w in (2, 3)):
            return p
    raise AssertionError("no candidate id lands on another shard in both world sizes")


@functools.lru_cache(maxsize=None)
def dataset(exact=True):
    """pid, pk, value: shared and never written to.  exact: values are
    eighths, so every sum is exact in any order; else uniform(-1, 6)."""
    rng = np.random.default_rng(41)
    pid = rng.integers(0, N_PID, N).astype(np.int64)
    w = np.arange(1, P_DATA + 1, dtype=np.float64) ** -1.1
    pk = rng.choice(P_DATA, size=N, p=w / w.sum()).astype(np.int64)
    value = rng.integers(-8, 49, N) / 8.0
    if not exact:
        value = rng.uniform(-1, 6, N)
    pid[:1100] = PID_WIDE
    pk[:1100] = np.arange(150, 1250)
    pid[1100:2300] = PID_DEEP
    pk[1100:2300] = 7
    # the smallest pair sum of the dataset, on another rank than PID_DEEP's
    # pair (the largest: 1200 records of a positive mean)
    pid[2300] = planted_pid()
    pk[2300] = 3
    value = value.copy()
    value[2300] = -64.0
    for a in (pid, pk, value):
        a.setflags(write=False)
    return dict(pid=pid, pk=pk, value=value)


def split(data, world, rank, how):
    """Record indices of one rank."""
    n = len(data["pid"])
    if how == "sorted":  # the records of the privacy ids this rank owns
        return np.nonzero(shard_np(data["pid"], world) == rank)[0]
    if how == "strided":
        return np.arange(rank, n, world)
    assert how == "rank0"  # rank 0 holds everything, the others nothing
    return np.arange(n) if rank == 0 else np.arange(0)


def plain(hs):
    """DatasetHistograms -> [(name, [[lower, upper, count, sum, max], ...])]."""
    return [(h.name.value, [[b.lower, b.upper, b.count, b.sum, b.max] for b in h.bins])
            for h in (hs.l0_contributions_histogram, hs.l1_contributions_histogram,
                      hs.linf_contributions_histogram, hs.linf_sum_contributions_histogram,
                      hs.count_per_partition_histogram, hs.count_privacy_id_per_partition)]


def plain_raw(int_bins, sum_count, sum_sum, sum_max, lowers):
    """The C ABI's bin arrays (numpy) in the same form."""
    from pipelinedp_amd.dataset_histograms import computing_histograms as ch
    ints = [ch._int_histogram(t, int_bins[i]) for i, t in enumerate(ch._INT_TYPES)]
    sums = ch._float_histogram(sum_count, sum_sum, sum_max, lowers)
    return [(h.name.value, [[b.lower, b.upper, b.count, b.sum, b.max] for b in h.bins])
            for h in ints[:3] + [sums] + ints[3:]]


def as_lists(want):
    """The oracle's output with every number a plain Python value."""
    return [(name, [[x.item() if hasattr(x, "item") else x for x in b] for b in bins])
            for name, bins in want]


def assert_same(got, want, tag):
    """tests/test_gpu_histograms.py::assert_same: integer histograms exact;
    LINF_SUM exact counts, and edges / sums / maxima to 1e-9 (pair sums that
    are not exactly representable depend on the summation order in the last
    ulp, and the edges follow their min / max)."""
    import pytest
    for (n1, b1), (n2, b2) in zip(got, want):
        assert n1 == n2
        assert len(b1) == len(b2), (tag, n1, len(b1), len(b2))
        for x, y in zip(b1, b2):
            if n1 == "linf_sum_contributions":
                assert x[2] == y[2], (tag, n1, x, y)
                for i in (0, 1, 3, 4):
                    assert x[i] == pytest.approx(y[i], rel=1e-9, abs=1e-9), (tag, n1, x, y)
            else:
                assert x == y, (tag, n1, x, y)
