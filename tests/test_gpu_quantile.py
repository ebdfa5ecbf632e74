"""dpg_quantile_keys + dpg_quantiles through the C ABI against the numpy
restatement of the walk (tests/percentile_ref.py), noise-free and with the
oracle's keyed node noise.  Every comparison also asserts that no branch of
the restated walk was decided by less than 1e-9, so that a last-bit
difference cannot hide behind (or cause) a mismatch."""
import numpy as np
import pytest
import torch

from tests import percentile_ref as ref

pytestmark = pytest.mark.gpu

SEED, NONCE = 77, 4242
P = 8
SIZES = (0, 1, 2, 17, 1000, 20000, 300, 40)  # kept values per partition
PK_OFFSET, PK_STRIDE = 5, 3
QS = (0.005, 0.1, 0.5, 0.9, 0.995)
QS6 = (0.02, 0.25, 0.4, 0.6, 0.75, 0.98)
NOISE_NONE, NOISE_LAPLACE, NOISE_GAUSSIAN = 0, 1, 2


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, SEED)
    yield c
    c.close()


def _records(lo, hi, centres):
    """Records of P partitions, shuffled, some of them not kept.  Partition 6
    is all-equal; partition 7 has values outside [lo, hi] and a NaN."""
    rng = np.random.default_rng(3)
    w = (hi - lo) / ref.L
    pk, val = [], []
    for k, m in enumerate(SIZES):
        leaves = rng.integers(0, ref.L, m)
        v = lo + (leaves + 0.5) * w if centres else leaves.astype(np.float64)
        if k == 6:
            v[:] = v[0]
        if k == 7:
            v[:5] = [lo - 10.0, hi + 10.0, hi, lo, np.nan]
        pk.append(np.full(m, k))
        val.append(v)
    pk, val = np.concatenate(pk).astype(np.int64), np.concatenate(val)
    # as many records that bounding dropped, with values that would move every quantile
    pk = np.concatenate([pk, pk])
    val = np.concatenate([val, np.full(len(val), lo)])
    keep = np.concatenate([np.ones(len(val) // 2, np.uint8), np.zeros(len(val) // 2, np.uint8)])
    o = rng.permutation(len(pk))
    return pk[o], val[o], keep[o]


RANGES = {"integers": (0.0, 65536.0, False), "centres": (-3.0, 7.0, True)}


@pytest.fixture(scope="module", params=list(RANGES))
def case(request):
    lo, hi, centres = RANGES[request.param]
    return (lo, hi) + _records(lo, hi, centres)


def _gpu(ctx, case, qs, kind=NOISE_NONE, scale=0.0, keep_partition=None):
    from pipelinedp_amd import _native
    lo, hi, pk, val, keep = case
    n = len(pk)
    qp = _native.fill(_native.QuantileParams, dict(
        lo=lo, hi=hi, noise_kind=kind, n_quantiles=len(qs), scale=float(scale),
        quantiles=list(qs), pk_offset=PK_OFFSET, pk_stride=PK_STRIDE, nonce=NONCE))
    d_pk, d_val = torch.from_numpy(pk).cuda(), torch.from_numpy(val).cuda()
    d_keep = torch.from_numpy(keep).cuda()
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    n_keys = torch.empty(1, dtype=torch.int64, device="cuda")
    ctx.quantile_keys(d_pk.data_ptr(), d_val.data_ptr(), d_keep.data_ptr(), n, P, qp,
                      keys.data_ptr(), n_keys.data_ptr(), None)
    out = torch.full((P, len(qs)), -777.0, dtype=torch.float64, device="cuda")
    kp = torch.from_numpy(keep_partition).cuda() if keep_partition is not None else None
    ctx.quantiles(keys.data_ptr(), n_keys.data_ptr(), P, qp,
                  kp.data_ptr() if kp is not None else None, out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), keys.cpu().numpy()[:int(n_keys.item())]


def _kept(case, k):
    lo, hi, pk, val, keep = case
    return val[(pk == k) & (keep == 1)]


def test_sorted_keys(ctx, case):
    lo, hi, pk, val, keep = case
    _, keys = _gpu(ctx, case, QS)
    m = (keep == 1) & ~np.isnan(val)
    want = np.sort((pk[m] << 16) | ref.leaf_of(val[m], lo, hi))
    assert np.array_equal(keys, want)


@pytest.mark.parametrize("qs", [QS, QS6], ids=["5", "6"])
def test_noise_free(ctx, case, qs):
    lo, hi = case[:2]
    got, _ = _gpu(ctx, case, qs)
    tol, leaf = 1e-12 * (hi - lo), (hi - lo) / ref.L
    for k in range(P):
        v = _kept(case, k)
        want, margin = ref.quantiles(v, qs, lo, hi)
        print(k, got[k], want, margin)
        assert margin >= 1e-9
        assert np.abs(got[k] - want).max() <= tol
        if len(v) == 0:  # an empty tree: the root's range
            assert np.abs(got[k] - (lo + np.array(qs) * (hi - lo))).max() <= tol
            continue
        for j, q in enumerate(qs):
            assert abs(got[k, j] - ref.order_statistic(v, q, lo, hi)) <= leaf


def test_degenerate_range(ctx):
    """lo == hi: every value is leaf 0 and every percentile is lo."""
    rng = np.random.default_rng(1)
    pk = rng.integers(0, P, 500).astype(np.int64)
    case = (2.5, 2.5, pk, rng.uniform(0, 5, 500), np.ones(500, np.uint8))
    got, keys = _gpu(ctx, case, QS)
    assert np.array_equal(keys, np.sort(pk << 16))
    assert (got == 2.5).all()


@pytest.mark.parametrize("kind", [NOISE_LAPLACE, NOISE_GAUSSIAN], ids=["laplace", "gaussian"])
def test_keyed_node_noise(ctx, case, kind):
    """A scale comparable to the counts: the alpha filter and the clamp at 0
    both fire; empty partitions walk their noise.  Partitions 2 and 5 are not
    kept: their rows stay untouched."""
    from oracle import oracle
    lo, hi = case[:2]
    scale = 6.0
    keep_partition = np.ones(P, np.uint8)
    keep_partition[[2, 5]] = 0
    got, _ = _gpu(ctx, case, QS, kind, scale, keep_partition)
    ss = oracle.stream_seed(SEED, NONCE)
    tol = 1e-12 * (hi - lo)
    stats = {}
    for k in range(P):
        if not keep_partition[k]:
            assert (got[k] == -777.0).all()
            continue
        noised = ref.oracle_noise(kind, scale, ss, PK_OFFSET + k * PK_STRIDE)
        want, margin = ref.quantiles(_kept(case, k), QS, lo, hi, noised, stats)
        print(k, got[k], want, margin)
        assert margin >= 1e-9
        assert np.abs(got[k] - want).max() <= tol
    assert stats["clamped"] > 0 and stats["filtered"] > 0
