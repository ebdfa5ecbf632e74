"""dpg_merge_pair_runs through the C ABI against numpy: the runs
concatenated, a stable argsort by pk (so a partition's entries are ordered by
run, then by position in the run) and searchsorted starts.  Everything is
integer placement and must be exact, byte for byte, on every execution."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF
TAIL = 5


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 13)
    yield c
    c.close()


def _entries(pk, rng):
    from pipelinedp_amd import pre_aggregation as pa
    n = len(pk)
    a = np.zeros(n, dtype=pa.PAIR_DTYPE)
    a["pk"] = pk
    a["count"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    a["sum"] = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    a["np"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    a["ncl"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return a


def _words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 3)


def _runs(pks, seed):
    """(entries of all runs concatenated, run_start) from one pk array per run."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum([len(p) for p in pks])]).astype(np.int64)
    pk = np.concatenate([np.asarray(p, np.int64) for p in pks]) if pks else np.zeros(0, np.int64)
    return _entries(pk, rng), start


def _model(a, P):
    order = np.argsort(a["pk"], kind="stable")
    return a[order], np.searchsorted(a["pk"][order], np.arange(P + 1)).astype(np.int64)


def _merge(ctx, a, run_start, P):
    n = len(a)
    d_in = torch.from_numpy(_words(a).view(np.int64).copy()).cuda()
    out = torch.full((n + TAIL, 3), SENTINEL, dtype=torch.int64, device="cuda")
    starts = torch.full((P + 1 + TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
    n_bad = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    ctx.merge_pair_runs(d_in.data_ptr(), run_start.tolist(), P, out.data_ptr(),
                        starts.data_ptr(), n_bad.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), starts.cpu().numpy(), n_bad.cpu().numpy()


def _sorted_draws(rng, P, n):
    return np.sort(rng.integers(0, P, n))


def _cases():
    rng = np.random.default_rng(99)
    c = {}
    c["all_empty"] = ([[], [], []], 50)
    c["one_run"] = ([_sorted_draws(rng, 300, 5000)], 300)
    c["middle_empty"] = ([_sorted_draws(rng, 97, 3000), [], _sorted_draws(rng, 97, 1000)], 97)
    # partition 7 is present in every one of 64 runs, among others
    c["in_every_run"] = ([np.sort(np.concatenate([[7] * (1 + r % 3), rng.integers(0, 40, 30)]))
                          for r in range(64)], 40)
    # one partition of 5000 pairs in a single run: it spans blocks of the grid
    c["long_partition"] = ([np.sort(np.concatenate([[11] * 5000, rng.integers(0, 30, 200)])),
                            _sorted_draws(rng, 30, 100)], 30)
    c["one_partition"] = ([[0] * 70, [0] * 3, [], [0] * 129], 1)
    c["sparse"] = ([np.sort(rng.integers(0, 100_000, 4)), [99_999], [0, 5, 99_999],
                    np.sort(rng.integers(0, 100_000, 2))], 100_000)
    # nruns x n_partitions = 64 x 100 + 1 > one 2048-entry scan chunk
    c["beyond_scan_chunk"] = ([_sorted_draws(rng, 100, 40 + r) for r in range(64)], 100)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_merge_equals_numpy(ctx, name):
    pks, P = CASES[name]
    a, run_start = _runs(pks, 7)
    n = len(a)
    if name == "sparse":
        assert n == 10
    want, want_starts = _model(a, P)
    out, starts, n_bad = _merge(ctx, a, run_start, P)
    assert n_bad.tolist() == [0, -5]
    assert np.array_equal(starts[:P + 1], want_starts)
    assert (starts[P + 1:] == SENTINEL).all()
    assert np.array_equal(out[:n], _words(want))
    assert (out[n:].view(np.int64) == SENTINEL).all()
    if name == "one_run":  # a copy
        assert np.array_equal(out[:n], _words(a))
    again, starts2, _ = _merge(ctx, a, run_start, P)
    assert again.tobytes() == out.tobytes() and starts2.tobytes() == starts.tobytes()


def test_bad_entries_are_counted_and_dropped(ctx):
    """Two out-of-range pks (one inside a run, one at a run's end) and one
    descent: n_bad == 3, the other entries placed as the model places the
    input without those three.  The bad entries sit where include/dpg.h
    promises that: between two partitions of their run, not inside one."""
    P = 60
    rng = np.random.default_rng(5)
    runs = [_sorted_draws(rng, P, 700).tolist() for _ in range(3)]

    def between(run, j):
        """The first position >= j whose neighbours belong to two partitions."""
        while not 0 < run[j - 1] < run[j + 1]:
            j += 1
        return j

    i0, i2 = between(runs[0], 300), between(runs[2], 400)
    runs[0][i0] = P + 5                   # out of range, inside run 0
    runs[1][-1] = 0xFFFFFFFF              # out of range, the last entry of run 1
    runs[2][i2] = runs[2][i2 - 1] - 1     # descends below its predecessor
    a, run_start = _runs(runs, 8)
    bad = np.zeros(len(a), bool)
    bad[[i0, 700 + 699, 1400 + i2]] = True
    want, want_starts = _model(a[~bad], P)
    out, starts, n_bad = _merge(ctx, a, run_start, P)
    assert n_bad[0] == 3
    assert np.array_equal(starts[:P + 1], want_starts) and starts[P] == len(a) - 3
    assert np.array_equal(out[:len(want)], _words(want))
    assert (out[len(want):].view(np.int64) == SENTINEL).all()


def test_unsorted_runs_leave_readable_starts(ctx):
    """Runs that are not ascending at all (the caller fails on n_bad, but only
    after it has read the result): n_bad > 0, partition_start ascends from 0
    to at most n, nothing is written behind the output."""
    P = 40
    rng = np.random.default_rng(6)
    runs = [rng.integers(0, P + 3, 3000).tolist() for _ in range(4)]
    a, run_start = _runs(runs, 9)
    n = len(a)
    out, starts, n_bad = _merge(ctx, a, run_start, P)
    pk = np.concatenate(runs)
    first = np.zeros(n, bool)
    first[run_start[:-1]] = True
    prev = np.concatenate([[0], pk[:-1]])
    bad = (pk >= P) | (~first & (prev < P) & (pk < prev))
    assert n_bad[0] == bad.sum() > 0
    s = starts[:P + 1]
    assert s[0] == 0 and (np.diff(s) >= 0).all() and s[P] <= n
    assert (starts[P + 1:] == SENTINEL).all()
    assert (out[n:].view(np.int64) == SENTINEL).all()


def test_stage_names(ctx):
    pks, P = CASES["middle_empty"]
    a, run_start = _runs(pks, 7)
    _merge(ctx, a, run_start, P)
    assert list(ctx.stage_times())[:3] == ["pairs:bounds", "pairs:scan", "pairs:merge"]


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    import ctypes
    buf = torch.full((3 * 64,), 7, dtype=torch.int64, device="cuda")
    out = torch.full((3 * 64,), 7, dtype=torch.int64, device="cuda")
    st = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p, o, s = buf.data_ptr(), out.data_ptr(), st.data_ptr()

    def rs(*v):
        return (ctypes.c_int64 * len(v))(*v)

    INVALID, UNSUPPORTED = 1, 5
    f = lib.dpg_merge_pair_runs
    assert f(h, p, rs(0, 2, 4), 0, 5, o, s, s, None) == INVALID
    assert f(h, p, rs(*range(67)), 65, 5, o, s, s, None) == INVALID
    assert f(h, p, None, 2, 5, o, s, s, None) == INVALID
    assert f(h, p, rs(1, 2, 4), 2, 5, o, s, s, None) == INVALID
    assert f(h, p, rs(0, 3, 2), 2, 5, o, s, s, None) == INVALID
    assert f(h, p, rs(0, 2, 4), 2, -1, o, s, s, None) == INVALID
    assert f(h, p, rs(0, 2, 4), 2, 5, o, None, s, None) == INVALID
    assert f(h, p, rs(0, 2, 4), 2, 5, o, s, None, None) == INVALID
    assert f(h, None, rs(0, 2, 4), 2, 5, o, s, s, None) == INVALID
    assert f(h, p, rs(0, 2, 4), 2, 5, None, s, s, None) == INVALID
    assert f(h, p, rs(0, 2, 4), 2, 5, p, s, s, None) == INVALID  # in place
    assert f(h, p, rs(0, 2, 2**31), 2, 5, o, s, s, None) == UNSUPPORTED
    assert f(h, p, rs(0, 2, 4), 2, 2**31, o, s, s, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 7).all() and (out == 7).all() and (st == 7).all()
