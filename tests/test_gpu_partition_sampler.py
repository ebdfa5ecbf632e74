"""GPU partition sampler (dpg_sample_partitions, csrc/dpg_sample.h) against
its definition, hashlib.sha1 over repr(key): the hash itself, the mask's bit
layout and zeroed tail, the unsigned 64-bit compare, the route
perform_utility_analysis takes for integer keys, and bad arguments."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import _native
from pipelinedp_amd import analysis
from pipelinedp_amd.analysis import utility_analysis as ua_mod
from tests import sampler_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend(built):
    return pdp.MI355XBackend(device=0, seed=7)


def sha(k) -> int:
    return int(hashlib.sha1(repr(int(k)).encode()).hexdigest()[:16], 16)


def sample(backend, n, bound, keys=None, key_lo=0, key_stride=1, want_hashes=False):
    """(mask bytes, hashes or None) of one dpg_sample_partitions call over a
    mask buffer pre-filled with ones."""
    dev = backend.device
    mask = torch.full((8 * max((n + 63) // 64, 1),), 0xFF, dtype=torch.uint8, device=dev)
    hashes = torch.zeros(max(n, 1), dtype=torch.int64, device=dev) if want_hashes else None
    kt = torch.from_numpy(np.asarray(keys, dtype=np.int64)).to(dev) if keys is not None else None
    sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    backend.ctx.sample_partitions(
        ctypes.c_void_p(kt.data_ptr()) if kt is not None else None, key_lo, key_stride, n, bound,
        ctypes.c_void_p(mask.data_ptr()),
        ctypes.c_void_p(hashes.data_ptr()) if hashes is not None else None, sptr)
    h = hashes.cpu().numpy().view(np.uint64)[:n] if hashes is not None else None
    return mask.cpu().numpy()[:8 * ((n + 63) // 64)], h


@pytest.fixture(scope="module")
def random_hashes(backend):
    """(keys, their hashlib hashes) of the seeded random keys: shared."""
    keys = sampler_keys.random_keys()
    return keys, [sha(k) for k in keys]


def test_hashes_equal_sha1_on_key_table(backend, random_hashes):
    keys = sampler_keys.edge_keys() + random_hashes[0]
    want = [sha(k) for k in sampler_keys.edge_keys()] + random_hashes[1]
    _, got = sample(backend, len(keys), 1 << 63, keys=keys, want_hashes=True)
    bad = [(k, int(g), w) for k, g, w in zip(keys, got, want) if int(g) != w]
    assert not bad, bad[:5]


def test_hashes_equal_sha1_on_dense_ids(backend):
    _, got = sample(backend, 10_000, 1 << 63, want_hashes=True)
    assert got.tolist() == [sha(k) for k in range(10_000)]


@pytest.mark.parametrize("lo,stride", [(0, 1), (3, 8), (5, 3)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100_003])
def test_mask_bits_and_zeroed_tail(backend, n, lo, stride):
    bound = ua_mod._sample_bound(0.5)
    got, _ = sample(backend, n, bound, key_lo=lo, key_stride=stride)   # pre-filled with 0xFF
    decisions = np.array([sha(lo + i * stride) < bound for i in range(n)], bool)
    want = np.zeros(8 * ((n + 63) // 64), np.uint8)
    packed = np.packbits(decisions, bitorder="little")
    want[:len(packed)] = packed
    np.testing.assert_array_equal(got, want)


def test_compare_is_64_bit_and_unsigned(backend, random_hashes):
    keys, hs = random_hashes
    pick = [next(i for i, h in enumerate(hs) if h >> 32 >= 1 << 31),
            next(i for i, h in enumerate(hs) if h >> 32 < 1 << 31 and h & 0xFFFFFFFF >= 1 << 31),
            next(i for i, h in enumerate(hs) if h >> 32 < 1 << 31 and h & 0xFFFFFFFF < 1 << 31)]
    for i in pick:
        k, h = keys[i], hs[i]
        assert sample(backend, 1, h, keys=[k])[0][0] == 0, (k, h)
        assert sample(backend, 1, h + 1, keys=[k])[0][0] == 1, (k, h)
    sub = keys[:1000]
    none, _ = sample(backend, len(sub), 0, keys=sub)
    assert not none.any()
    every, _ = sample(backend, len(sub), 1 << 64, keys=sub)        # keep_all
    want = np.zeros(8 * ((len(sub) + 63) // 64), np.uint8)
    want[:len(sub) // 8] = 0xFF
    np.testing.assert_array_equal(every, want)


def test_sample_bound_reaches_two_to_64():
    assert ua_mod._sample_bound(1 - 2**-60) == 2**64


# ------------------------------------------------------------- engine route
def _engine_keys(cols, extractors, prob):
    params = pdp.AggregateParams(noise_kind=pdp.NoiseKind.LAPLACE, metrics=[pdp.Metrics.COUNT],
                                 max_partitions_contributed=2, max_contributions_per_partition=1)
    opts = analysis.UtilityAnalysisOptions(epsilon=1.0, delta=1e-6, aggregate_params=params,
                                           partitions_sampling_prob=prob)
    _, per = analysis.perform_utility_analysis(cols, pdp.MI355XBackend(device=0, seed=7), opts,
                                               extractors)
    return {key for (key, _), _ in per}


def _sparse_columns():
    rng = np.random.default_rng(77)
    universe = np.unique(rng.integers(-2**62, 2**62, 5000))      # sparse, partly negative
    assert (universe < 0).any() and (universe > 0).any()
    n = 50_000
    pk = universe[rng.integers(0, len(universe), n)]
    pid = rng.integers(0, 3000, n)
    return pid, pk


def test_engine_takes_the_device_route_for_integer_keys(built, monkeypatch):
    pid, pk = _sparse_columns()
    prob = 0.3
    bound = ua_mod._sample_bound(prob)
    want = {int(k) for k in np.unique(pk) if ua_mod._keep_by_hash(int(k), bound)}
    assert 0 < len(want) < len(np.unique(pk))
    cols = pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                            value=torch.ones(len(pk), dtype=torch.float64))
    ex = pdp.DataExtractors("pid", "pk", "value")
    assert _engine_keys(cols, ex, prob) == want

    def no_host_hash(key, bound):
        raise AssertionError("the host sampler was called for an integer key")

    monkeypatch.setattr(ua_mod, "_keep_by_hash", no_host_hash)
    assert _engine_keys(cols, ex, prob) == want


def test_engine_keeps_the_host_route_for_string_keys(built, monkeypatch):
    calls = []
    real = ua_mod._keep_by_hash

    def spy(key, bound):
        calls.append(key)
        return real(key, bound)

    monkeypatch.setattr(ua_mod, "_keep_by_hash", spy)
    rows = [(i % 50, f"pk{i % 120}", 1.0) for i in range(2000)]
    ex = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                            value_extractor=lambda r: r[2])
    prob = 0.5
    bound = ua_mod._sample_bound(prob)
    got = _engine_keys(rows, ex, prob)
    assert got == {f"pk{i}" for i in range(120) if real(f"pk{i}", bound)}
    assert sorted(calls) == sorted(f"pk{i}" for i in range(120))


# ------------------------------------------------------------ bad arguments
def test_bad_arguments(backend):
    ctx = backend.ctx
    dev = backend.device
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda n, mask: ctx.lib.dpg_sample_partitions(
        ctx.handle, None, 0, 1, n, ctypes.c_uint64(1 << 63), 0, mask, None, sptr)
    assert buf.data_ptr() % 8 == 0
    assert call(-1, ctypes.c_void_p(buf.data_ptr())) == 1          # DPG_ERR_INVALID_ARG
    assert call(10, None) == 1
    assert call(10, ctypes.c_void_p(buf.data_ptr() + 4)) == 1
    assert call(10, ctypes.c_void_p(buf.data_ptr())) == _native.DPG_OK
    torch.cuda.synchronize()
