"""dpg_sort_pairs_u64 through the C ABI: the result equals numpy's stable
argsort exactly, the payload (the input index) shows stability, at the sizes
where the tiling changes path and for keys that make passes skip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 2048  # DPG_SHARD_TILE
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)
KINDS = ("equal", "top_byte", "random", "few")


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys():
    """One host array per kind of the largest size; every case takes a prefix."""
    n = max(SIZES)
    rng = np.random.default_rng(5)
    few = rng.integers(0, 2**64, 16, dtype=np.uint64)
    return dict(
        equal=np.full(n, 0x0123456789ABCDEF, dtype=np.uint64),
        top_byte=(rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x1234),
        random=rng.integers(0, 2**64, n, dtype=np.uint64),
        few=few[rng.integers(0, 16, n)])


def _sort(ctx, k, begin, end, with_vals=True):
    n = len(k)
    d_k = torch.from_numpy(k.view(np.int64)).cuda()
    d_v = torch.arange(n, dtype=torch.int32, device="cuda")
    # sentinels: entries the sort must overwrite (or, for n = 0, leave alone)
    o_k = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    o_v = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    ctx.sort_pairs_u64(d_k.data_ptr(), d_v.data_ptr() if with_vals else None, n, begin, end,
                       o_k.data_ptr(), o_v.data_ptr() if with_vals else None, None)
    torch.cuda.synchronize()
    return o_k.cpu().numpy().view(np.uint64), o_v.cpu().numpy()


def _digits(k, begin, end):
    if end - begin == 64:
        return k
    return (k >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_full_sort_is_numpy_stable_argsort(ctx, keys, kind, n):
    k = keys[kind][:n]
    got_k, got_v = _sort(ctx, k, 0, 64)
    if n == 0:
        assert got_k[0] == np.uint64(-7 & (2**64 - 1)) and got_v[0] == -7
        return
    order = np.argsort(k, kind="stable")
    assert np.array_equal(got_v[:n], order.astype(np.int32))
    assert np.array_equal(got_k[:n], k[order])


@pytest.mark.parametrize("bits", [(0, 0), (0, 8), (8, 24), (5, 18), (56, 64), (32, 64), (3, 64)])
def test_bit_ranges(ctx, keys, bits):
    """Only the bits [begin, end) order the output; equal digits keep their
    input order."""
    begin, end = bits
    k = keys["random"]
    got_k, got_v = _sort(ctx, k, begin, end)
    order = np.argsort(_digits(k, begin, end), kind="stable")
    assert np.array_equal(got_v, order.astype(np.int32))
    assert np.array_equal(got_k, k[order])


def test_keys_only(ctx, keys):
    k = keys["random"][:T + 65]
    got_k, got_v = _sort(ctx, k, 0, 64, with_vals=False)
    assert np.array_equal(got_k, np.sort(k))
    assert (got_v == -7).all()


def test_argument_checks(ctx):
    from pipelinedp_amd import _native
    a = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(_native.NativeError, match="unsupported"):
        ctx.sort_pairs_u64(a.data_ptr(), None, 2**31, 0, 64, a.data_ptr(), None, None)
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.sort_pairs_u64(a.data_ptr(), None, 8, 0, 64, a.data_ptr(), None, None)  # in place
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.sort_pairs_u64(a.data_ptr(), None, 8, 9, 8, a.data_ptr(), None, None)
