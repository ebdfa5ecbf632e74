"""dpg_vector_clip_noise through the C ABI: the norm clip against its numpy
restatement (tests/vector_ref.py) and the per-coordinate noise against the
oracle's keyed sampler, at the tolerance tests/test_gpu_parity.py grants the
device sampler (one granule)."""
import numpy as np
import pytest
import torch

from tests import vector_ref as ref

pytestmark = pytest.mark.gpu

SEED, NONCE = 91, 777
P = 24
ZERO_ROW = 5
PK_OFFSET, PK_STRIDE = 7, 3
SENTINEL = -777.0


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, SEED)
    yield c
    c.close()


def _sums(D):
    s = np.random.default_rng(D).integers(-20, 21, (P, D)).astype(np.float64)
    s[ZERO_ROW] = 0.0
    return s


def _gpu(ctx, sums, norm_kind, max_norm, noise_kind=ref.NOISE_NONE, scale=0.0,
         keep_partition=None, in_place=False):
    from pipelinedp_amd import _native
    vp = _native.fill(_native.VectorParams, dict(
        size=sums.shape[1], norm_kind=norm_kind, max_norm=float(max_norm), noise_kind=noise_kind,
        scale=float(scale), pk_offset=PK_OFFSET, pk_stride=PK_STRIDE, nonce=NONCE))
    d_sums = torch.from_numpy(sums).cuda()
    out = d_sums if in_place else torch.full(sums.shape, SENTINEL, dtype=torch.float64,
                                             device="cuda")
    kp = torch.from_numpy(keep_partition).cuda() if keep_partition is not None else None
    ctx.vector_clip_noise(d_sums.data_ptr(), P, vp, kp.data_ptr() if kp is not None else None,
                          out.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _max_norm(sums, kind):
    """LINF: 10 (entries reach 20); L1 / L2: the median of the rows' norms, so
    that some rows are scaled and some are not."""
    if kind == ref.NORM_LINF:
        return 10.0
    norms = np.array([ref.norm(r, kind) for r in sums])
    m = float(np.median(norms))
    assert (norms > m).any() and (norms <= m).any()
    return m


@pytest.mark.parametrize("D", [3, 100])
@pytest.mark.parametrize("kind", [ref.NORM_LINF, ref.NORM_L1, ref.NORM_L2],
                         ids=["linf", "l1", "l2"])
@pytest.mark.parametrize("in_place", [False, True], ids=["copy", "alias"])
def test_clip_without_noise(ctx, D, kind, in_place):
    sums = _sums(D)
    max_norm = _max_norm(sums, kind)
    got = _gpu(ctx, sums, kind, max_norm, in_place=in_place)
    want = np.stack([ref.clip(r, max_norm, kind) for r in sums])
    print(D, kind, np.abs(got - want).max())
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-12 * max_norm
    assert (got[ZERO_ROW] == 0.0).all()
    if kind != ref.NORM_LINF:  # rows inside the ball pass unchanged
        inside = np.array([ref.norm(r, kind) <= max_norm for r in sums])
        assert np.array_equal(got[inside], sums[inside])


@pytest.mark.parametrize("D", [3, 100])
@pytest.mark.parametrize("noise", [ref.NOISE_LAPLACE, ref.NOISE_GAUSSIAN],
                         ids=["laplace", "gaussian"])
def test_keyed_noise_and_skipped_partitions(ctx, D, noise):
    from oracle import oracle
    sums = _sums(D)
    kind = ref.NORM_L2
    max_norm = _max_norm(sums, kind)
    scale = 2.5
    keep_partition = np.ones(P, np.uint8)
    keep_partition[[2, 11]] = 0
    got = _gpu(ctx, sums, kind, max_norm, noise, scale, keep_partition)
    ss = oracle.stream_seed(SEED, NONCE)
    moved = 0
    for k in range(P):
        if not keep_partition[k]:
            assert (got[k] == SENTINEL).all()
            continue
        clipped = ref.clip(sums[k], max_norm, kind)
        noised = ref.oracle_noise(noise, scale, ss, PK_OFFSET + PK_STRIDE * k)
        want = np.array([noised(d, clipped[d]) for d in range(D)])
        assert np.allclose(got[k], want, rtol=1e-12, atol=1e-6), (k, got[k], want)
        moved += int((np.abs(got[k] - clipped) > 1e-3).sum())
    assert moved > 0.5 * (P - 2) * D  # the noise is there


def test_argument_errors(ctx):
    from pipelinedp_amd import _native
    lib, h = ctx.lib, ctx.handle
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    INVALID, UNSUPPORTED = 1, 5

    def params(**kw):
        f = dict(size=2, norm_kind=ref.NORM_L2, max_norm=1.0, noise_kind=0, scale=0.0,
                 pk_offset=0, pk_stride=1, nonce=0)
        f.update(kw)
        return _native.fill(_native.VectorParams, f)
    assert lib.dpg_vector_clip_noise(h, None, 4, params(), None, p, None) == INVALID
    assert lib.dpg_vector_clip_noise(h, p, 4, params(), None, None, None) == INVALID
    assert lib.dpg_vector_clip_noise(h, p, 4, None, None, p, None) == INVALID
    assert lib.dpg_vector_clip_noise(h, p, 4, params(size=0), None, p, None) == INVALID
    assert lib.dpg_vector_clip_noise(h, p, 4, params(norm_kind=3), None, p, None) == INVALID
    assert lib.dpg_vector_clip_noise(h, p, 1, params(size=_native.VECTOR_MAX_SIZE + 1), None, p,
                                     None) == UNSUPPORTED
    torch.cuda.synchronize()
