"""The exact noise reference (tests/noise_ref.py) against the C oracle, the
granularity rule on both, and the distribution of the reference itself.  No
GPU: tests/test_gpu_noise_exact.py pins the device to the same reference
sample by sample.

A sample of the oracle may differ from the reference by one granule per
rounding of a transcendental result (floor twice for Laplace, rint once for
Gaussian), never more, and only on a small share of the samples: with
functions good to about 2 ulp the value in front of the rounding, about
2^40 t, moves by about 2^-12 |t| granules, a share of a few 1e-4.  The cap is
0.5 %."""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

from oracle import oracle
from tests import noise_ref as nr

from tests.noise_ref import BOUND, MAX_SHARE, SCALES, step_ulps, values_for

SSEED = 0x0DDBA11C0FFEE123
N = 4000


def test_ties_are_ties():
    for scale in SCALES:
        g = nr.granularity(scale)
        xs = values_for(scale)
        assert [nr.snap_index(x, g) for x in xs[3:7]] == [6, 8, -2 ** 20, -2 ** 20 - 2]


def test_philox_and_seed_restatements():
    assert nr.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C,
                                                     0x9B00DBD8]
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        k = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        assert nr.philox4x32_10(c, k) == oracle.philox(c, k)
        seed, nonce = (int(v) for v in rng.integers(0, 2 ** 64, 2, dtype=np.uint64))
        assert nr.stream_seed(seed, nonce) == oracle.stream_seed(seed, nonce)
    assert nr.stream_seed(2 ** 64 - 1, 2 ** 64 - 1) == oracle.stream_seed(2 ** 64 - 1, 2 ** 64 - 1)


def test_u53_double_is_the_rational_below_half():
    # w < 2^52: w + 0.5 is a double; above, it rounds to even (at most 2^-54 off)
    assert nr.u53_double(0x7FFFFFFF, 0xFFFFF800) == float(nr.u53(0x7FFFFFFF, 0xFFFFF800))
    assert nr.u53_double(0, 0) == 2.0 ** -54
    top = nr.u53(0xFFFFFFFF, 0xFFFFFFFF)
    assert top == 1 - Fraction(1, 2 ** 54) and nr.u53_double(0xFFFFFFFF, 0xFFFFFFFF) == 1.0


@pytest.mark.parametrize("kind", [nr.NOISE_LAPLACE, nr.NOISE_GAUSSIAN], ids=["laplace", "gaussian"])
@pytest.mark.parametrize("scale", SCALES, ids=[s.hex() for s in SCALES])
def test_oracle_matches_the_exact_reference(kind, scale):
    xs = values_for(scale)
    g = nr.granularity(scale)
    differing = 0
    for k in range(N):
        x = xs[k % len(xs)]
        pk = k if k % 3 else k + (7 << 32)  # both counter words
        slot = k % 4
        got = oracle.noise_sample(kind, x, scale, SSEED, pk, slot)
        want, n = nr.noise_sample(kind, x, scale, SSEED, pk, slot)
        assert nr.on_lattice(got, g), (k, x, got)
        d = nr.index_offset(got, n, g, BOUND[kind])
        assert d is not None, (k, x, got, want)
        assert (d == 0) == (got == want)
        differing += d != 0
    print(f"kind {kind} scale {scale.hex()}: {differing} of {N} samples differ")
    assert differing <= MAX_SHARE * N, differing


def _granularity_probes():
    out = []
    for k in (-30, -1, 0, 1, 10, 40, 41, 60):
        p = 2.0 ** k
        out += [p, 1.5 * p] + [step_ulps(p, d) for d in (-4, -1, 1, 4)]
    rng = np.random.default_rng(11)
    out += [float(m * 2.0 ** e) for m, e in zip(rng.uniform(1.0, 2.0, 2000),
                                                 rng.integers(-60, 61, 2000))]
    return out


def test_reference_granularity_is_the_smallest_power_of_two():
    for s in _granularity_probes():
        g = nr.granularity(s)
        target = Fraction(s) / 2 ** 40
        assert g.numerator == 1 or g.denominator == 1
        assert g / 2 < target <= g, s.hex()


def test_oracle_granularity_is_exact():
    bad = [s.hex() for s in _granularity_probes()
           if oracle.granularity(s) != float(nr.granularity(s))]
    assert not bad, bad


def _reference_samples(kind, scale, n=20000):
    return np.array([nr.noise_sample(kind, 0.0, scale, 12345, k, 0)[0] for k in range(n)])


def _masses(values, sigma, p1, p12):
    d = np.abs(values)
    w1 = np.mean(d <= sigma)
    w12 = np.mean((d > sigma) & (d <= 2 * sigma))
    assert abs(w1 - p1) < 4 * math.sqrt(p1 * (1 - p1) / len(values))
    assert abs(w12 - p12) < 4 * math.sqrt(p12 * (1 - p12) / len(values))


DIST_SCALES = [2.0 ** -20, 3.7, 1e12]


@pytest.mark.parametrize("scale", DIST_SCALES, ids=[s.hex() for s in DIST_SCALES])
def test_reference_laplace_distribution(scale):
    v = _reference_samples(nr.NOISE_LAPLACE, scale)
    assert stats.ks_1samp(v, stats.laplace(loc=0.0, scale=scale).cdf).pvalue > 1e-4
    _masses(v, math.sqrt(2) * scale, 1 - math.exp(-math.sqrt(2)),
            math.exp(-math.sqrt(2)) - math.exp(-2 * math.sqrt(2)))


@pytest.mark.parametrize("scale", DIST_SCALES, ids=[s.hex() for s in DIST_SCALES])
def test_reference_gaussian_distribution(scale):
    v = _reference_samples(nr.NOISE_GAUSSIAN, scale)
    assert stats.ks_1samp(v, stats.norm(loc=0.0, scale=scale).cdf).pvalue > 1e-4
    _masses(v, scale, 0.68268949213, 0.27181024396)
