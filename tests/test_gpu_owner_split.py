"""dpg_owner_split_keys through the C ABI against numpy (a stable argsort of
pk % R, a bincount, the re-based keys): everything exact.  Shapes: empty
inputs, one key, the wave and tile edges, a device count below n_max (the
tails of the outputs must survive), R x tiles beyond one scan chunk, and one
rank (keys unchanged)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 1000
SENTINEL_KEY, SENTINEL_SRC = -0x0123456789ABCDEF, 0x7EADBEEF
# (n_keys, n_max, R)
SHAPES = [(0, 0, 2), (0, 4096, 8), (1, 1, 2),
          (63, 63, 3), (64, 64, 3), (65, 65, 3),
          (2047, 2047, 8), (2048, 2048, 8), (2049, 2049, 8),  # DPG_SHARD_TILE
          (4097, 5000, 5),
          (70_000, 70_000, 64),  # R x tiles = 2240 > one 2048-entry scan chunk
          (50_000, 50_000, 1)]


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    assert _native.SHARD_TILE == 2048 and _native.SHARD_MAX_RANKS == 64
    c = _native.Context(0, 11)
    yield c
    c.close()


def _inputs(n, R, low_bits):
    """name -> uint64 keys pk << low_bits | low."""
    rng = np.random.default_rng(1000 * n + 10 * R + low_bits)
    low = rng.integers(0, 1 << 16, n).astype(np.uint64) if low_bits else np.zeros(n, np.uint64)
    lb = np.uint64(low_bits)

    def keys(pk):
        return (pk.astype(np.uint64) << lb) | low

    pk = rng.integers(0, P, n)
    i = np.arange(n)
    return {"random": keys(pk), "sorted": np.sort(keys(pk)),
            # all keys share one owner (the last rank), partitions differ
            "one_owner": keys((i % 7) * R + (R - 1)),
            # consecutive keys have consecutive owners: with R = 64 every lane
            # of a wave has another one
            "lane_owner": keys(i % P)}


def _model(keys, low_bits, R):
    lb, r = np.uint64(low_bits), np.uint64(R)
    pk = keys >> lb
    dest = (pk % r).astype(np.int64)
    order = np.argsort(dest, kind="stable")
    rebased = ((pk // r) << lb) | (keys & np.uint64((1 << low_bits) - 1))
    return rebased[order], order, np.bincount(dest, minlength=R)


def _split(ctx, keys, n_keys, n_max, low_bits, R, with_src):
    buf = np.full(max(n_max, 1), 0xFFFF_FFFF_FFFF, np.uint64)  # the tail: keys nobody may read
    buf[:n_keys] = keys
    d_keys = torch.from_numpy(buf.view(np.int64)).cuda()
    d_n = torch.tensor([n_keys], dtype=torch.int64, device="cuda")
    out = torch.full((max(n_max, 1),), SENTINEL_KEY, dtype=torch.int64, device="cuda")
    src = torch.full((max(n_max, 1),), SENTINEL_SRC, dtype=torch.int32, device="cuda")
    counts = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    ctx.owner_split_keys(d_keys.data_ptr(), d_n.data_ptr(), n_max, low_bits, R, out.data_ptr(),
                         src.data_ptr() if with_src else None, counts.data_ptr(), None)
    torch.cuda.synchronize()
    return (out.cpu().numpy().view(np.uint64), src.cpu().numpy(), counts.cpu().numpy())


@pytest.mark.parametrize("with_src", [True, False], ids=["src", "nosrc"])
@pytest.mark.parametrize("low_bits", [16, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_split_equals_numpy(ctx, shape, low_bits, with_src):
    n, n_max, R = shape
    for name, keys in _inputs(n, R, low_bits).items():
        want, order, want_counts = _model(keys, low_bits, R)
        out, src, counts = _split(ctx, keys, n, n_max, low_bits, R, with_src)
        assert np.array_equal(counts, want_counts), name
        assert np.array_equal(out[:n], want), name
        # past the device count nothing is written
        assert (out[n:].view(np.int64) == SENTINEL_KEY).all(), name
        if with_src:
            assert np.array_equal(src[:n], order), name
            assert (src[n:] == SENTINEL_SRC).all(), name
        else:
            assert (src == SENTINEL_SRC).all(), name
        if R == 1:
            assert np.array_equal(out[:n], keys), name


def test_stage_names(ctx):
    keys = _inputs(5000, 4, 16)["random"]
    _split(ctx, keys, 5000, 5000, 16, 4, True)
    assert list(ctx.stage_times())[:3] == ["owner:count", "owner:scan", "owner:scatter"]


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    INVALID, UNSUPPORTED = 1, 5
    assert lib.dpg_owner_split_keys(h, p, p, 4, 16, 0, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, 4, 16, 65, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, 4, 33, 2, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, 4, -1, 2, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, -1, 16, 2, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, None, 4, 16, 2, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, 4, 16, 2, p, p, None, None) == INVALID
    assert lib.dpg_owner_split_keys(h, None, p, 4, 16, 2, p, p, p, None) == INVALID
    assert lib.dpg_owner_split_keys(h, p, p, 2**31, 16, 2, p, p, p, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 7).all()  # the device was not touched
