"""dpg_vector_index + dpg_vector_sums through the C ABI against numpy: exact
on integer-valued rows, bitwise reproducible and within the summation-order
tolerance on float rows, with two partitions that each span several chunks
of DPG_VSUM_CHUNK sorted rows (head, whole-chunk and tail partials) among
small ones (direct stores) and empty ones."""
import numpy as np
import pytest
import torch

from tests import vector_ref as ref

pytestmark = pytest.mark.gpu

P, N = 40, 6000
EMPTY = (0, 17, 39)
DIMS = (1, 3, 16, 100)  # degenerate, not a power of two, one 128-byte row, the coordinate loop


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 11)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    """pk, the keep mask and the record index: 2000 records each in
    partitions 3 and 4, the rest spread over the others but 0, 17 and 39."""
    rng = np.random.default_rng(5)
    others = np.array([k for k in range(P) if k not in EMPTY + (3, 4)])
    pk = np.concatenate([np.full(2000, 3), np.full(2000, 4), rng.choice(others, N - 4000)])
    pk = pk[rng.permutation(N)].astype(np.int64)
    keep = (rng.random(N) < 0.7).astype(np.uint8)
    for k in (3, 4):  # at least two chunk edges inside each
        assert ((pk == k) & (keep == 1)).sum() > 2 * ref.VSUM_CHUNK
    return pk, keep


def _index(ctx, pk, keep, n_partitions=P):
    n = len(pk)
    d_pk, d_keep = torch.from_numpy(pk).cuda(), torch.from_numpy(keep).cuda()
    keys = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    n_keys = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    ctx.vector_index(d_pk.data_ptr() if n else None, d_keep.data_ptr() if n else None, n,
                     n_partitions, keys.data_ptr(), n_keys.data_ptr(), None)
    return keys, n_keys


def _sums(ctx, keys, n_keys, value, n_partitions=P):
    n, D = value.shape
    d_val = torch.from_numpy(value).cuda()
    out = torch.full((n_partitions, D), -777.0, dtype=torch.float64, device="cuda")
    ctx.vector_sums(keys.data_ptr(), n_keys.data_ptr(), d_val.data_ptr() if n else None, n, D,
                    n_partitions, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_index_is_the_sorted_kept_keys(ctx, records):
    pk, keep = records
    keys, n_keys = _index(ctx, pk, keep)
    torch.cuda.synchronize()
    m = keep == 1
    want = np.sort((pk[m] << 31) | np.arange(N, dtype=np.int64)[m])
    assert int(n_keys.item()) == len(want)
    assert np.array_equal(keys.cpu().numpy()[:len(want)], want)


@pytest.mark.parametrize("D", DIMS)
def test_integer_rows_are_exact(ctx, records, D):
    pk, keep = records
    value = np.random.default_rng(D).integers(-3, 14, (N, D)).astype(np.float64)
    keys, n_keys = _index(ctx, pk, keep)
    got = _sums(ctx, keys, n_keys, value)
    want = ref.partition_sums(pk, value, keep, P)
    assert np.array_equal(got, want)
    assert (got[list(EMPTY)] == 0.0).all()
    assert np.abs(got[[3, 4]]).sum() > 0


@pytest.mark.parametrize("mask", ["all", "none"])
def test_keep_all_and_keep_none(ctx, records, mask):
    pk, _ = records
    keep = np.ones(N, np.uint8) if mask == "all" else np.zeros(N, np.uint8)
    value = np.random.default_rng(2).integers(-3, 14, (N, 3)).astype(np.float64)
    keys, n_keys = _index(ctx, pk, keep)
    got = _sums(ctx, keys, n_keys, value)
    assert int(n_keys.item()) == (N if mask == "all" else 0)
    assert np.array_equal(got, ref.partition_sums(pk, value, keep, P))


def test_no_records(ctx):
    keys, n_keys = _index(ctx, np.zeros(0, np.int64), np.zeros(0, np.uint8))
    got = _sums(ctx, keys, n_keys, np.zeros((0, 3)))
    assert int(n_keys.item()) == 0
    assert got.shape == (P, 3) and (got == 0.0).all()


@pytest.mark.parametrize("D", DIMS)
def test_float_rows_reproducible_and_close(ctx, records, D):
    pk, keep = records
    value = np.random.default_rng(100 + D).uniform(-1.0, 1.0, (N, D))
    keys, n_keys = _index(ctx, pk, keep)
    a = _sums(ctx, keys, n_keys, value)
    keys2, n_keys2 = _index(ctx, pk, keep)
    b = _sums(ctx, keys2, n_keys2, value)
    assert a.tobytes() == b.tobytes()
    want = ref.partition_sums(pk, value, keep, P)
    bound = 1e-12 * ref.partition_sums(pk, np.abs(value), keep, P)  # summation order only
    err = np.abs(a - want)
    print(D, (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()


def test_argument_errors(ctx):
    from pipelinedp_amd import _native
    lib, h = ctx.lib, ctx.handle
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    val = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    INVALID, UNSUPPORTED = 1, 5
    # null pointers
    assert lib.dpg_vector_index(h, None, p, 4, P, p, p, None) == INVALID
    assert lib.dpg_vector_index(h, p, p, 4, P, p, None, None) == INVALID
    assert lib.dpg_vector_sums(h, p, None, val.data_ptr(), 4, 2, P, val.data_ptr(), None) == INVALID
    assert lib.dpg_vector_sums(h, p, p, val.data_ptr(), 4, 2, P, None, None) == INVALID
    assert lib.dpg_vector_sums(h, p, p, None, 4, 2, P, val.data_ptr(), None) == INVALID
    # the vector size
    assert lib.dpg_vector_sums(h, p, p, val.data_ptr(), 4, 0, P, val.data_ptr(), None) == INVALID
    assert lib.dpg_vector_sums(h, p, p, val.data_ptr(), 4, _native.VECTOR_MAX_SIZE + 1, 1,
                               val.data_ptr(), None) == UNSUPPORTED
    # n >= 2^31
    assert lib.dpg_vector_index(h, p, p, 2**31, P, p, p, None) == UNSUPPORTED
    assert lib.dpg_vector_sums(h, p, p, val.data_ptr(), 2**31, 2, P, val.data_ptr(), None) == UNSUPPORTED
    with pytest.raises(_native.NativeError, match="unsupported"):
        ctx.vector_index(p, p, 2**31, P, p, p, None)
    torch.cuda.synchronize()
