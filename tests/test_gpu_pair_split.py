"""dpg_owner_split_pairs through the C ABI against numpy (a stable argsort of
pk % R, a bincount, pk // R): the full 24 bytes of every entry compared as
integers, everything exact.  Shapes: empty input, one pair, the wave and tile
edges, several tiles with a ragged end, R x tiles beyond one scan chunk, and
one rank (a copy)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 1000
SENTINEL = -0x0123456789ABCDEF
# (n, R)
SHAPES = [(0, 2), (1, 2),
          (63, 3), (64, 3), (65, 3),
          (2047, 8), (2048, 8), (2049, 8),  # DPG_SHARD_TILE
          (3 * 2048 + 17, 5),
          (70_000, 64),  # R x tiles = 2240 > one 2048-entry scan chunk
          (50_000, 1)]
TAIL = 5  # sentinel entries behind the output


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    assert _native.SHARD_TILE == 2048 and _native.SHARD_MAX_RANKS == 64
    c = _native.Context(0, 11)
    yield c
    c.close()


def _entries(pk, rng):
    """Structured pair entries with the given pk: every other byte random,
    sums with every bit pattern (NaNs included), the leader bit on a third."""
    from pipelinedp_amd import pre_aggregation as pa
    n = len(pk)
    a = np.zeros(n, dtype=pa.PAIR_DTYPE)
    a["pk"] = pk
    a["count"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    a["sum"] = rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    a["np"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    lead = (rng.integers(0, 3, n) == 0).astype(np.uint32) << np.uint32(31)
    a["ncl"] = rng.integers(0, 1 << 31, n, dtype=np.uint64).astype(np.uint32) | lead
    return a


def _inputs(n, R):
    rng = np.random.default_rng(1000 * n + R)
    pk = rng.integers(0, P, n)
    i = np.arange(n)
    layouts = {"random": pk, "sorted": np.sort(pk),
               # all pairs share one owner (the last rank), partitions differ
               "one_owner": (i % 7) * R + (R - 1),
               # consecutive pairs have consecutive owners: with R = 64 every
               # lane of a wave has another one
               "lane_owner": i % P}
    return {k: _entries(v, rng) for k, v in layouts.items()}


def _words(a):
    """[n, 3] uint64 view of structured entries."""
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 3)


def _model(a, R):
    dest = (a["pk"] % R).astype(np.int64)
    order = np.argsort(dest, kind="stable")
    want = a[order].copy()
    want["pk"] //= R
    return want, np.bincount(dest, minlength=R)


def _split(ctx, a, R):
    n = len(a)
    d_in = torch.from_numpy(_words(a).view(np.int64).copy()).cuda()
    out = torch.full((n + TAIL, 3), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((R + 1,), -5, dtype=torch.int64, device="cuda")
    ctx.owner_split_pairs(d_in.data_ptr(), n, R, out.data_ptr(), counts.data_ptr(), None)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), counts.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_split_equals_numpy(ctx, shape):
    n, R = shape
    for name, a in _inputs(n, R).items():
        want, want_counts = _model(a, R)
        out, counts = _split(ctx, a, R)
        assert np.array_equal(counts[:R], want_counts), name
        assert counts[R] == -5, name
        assert np.array_equal(out[:n], _words(want)), name
        assert (out[n:].view(np.int64) == SENTINEL).all(), name  # nothing written behind
        if R == 1:
            assert np.array_equal(out[:n], _words(a)), name
        if n >= 63:  # the leader bit is set on some entries and clear on others
            assert 0 < int((a["ncl"] >> 31).sum()) < n, name


def test_stage_names(ctx):
    a = _inputs(5000, 4)["sorted"]
    _split(ctx, a, 4)
    names = list(ctx.stage_times())
    assert names[:3] == ["pairs:count", "pairs:scan", "pairs:owner_split"]


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = torch.full((3 * 64,), 7, dtype=torch.int64, device="cuda")
    out = torch.full((3 * 64,), 7, dtype=torch.int64, device="cuda")
    cnt = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p, o, c = buf.data_ptr(), out.data_ptr(), cnt.data_ptr()
    INVALID, UNSUPPORTED = 1, 5
    assert lib.dpg_owner_split_pairs(h, p, 4, 0, o, c, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, p, 4, 65, o, c, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, p, -1, 2, o, c, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, p, 4, 2, o, None, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, None, 4, 2, o, c, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, p, 4, 2, None, c, None) == INVALID
    assert lib.dpg_owner_split_pairs(h, p, 4, 2, p, c, None) == INVALID  # in place
    assert lib.dpg_owner_split_pairs(h, p, 2**31, 2, o, c, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 7).all() and (out == 7).all() and (cnt == 7).all()  # the device was not touched
