"""An exact reference of the noise and selection arithmetic of k_select_noise
(csrc/dpg_select.h, samplers in csrc/dpg_common.h), independent of the C
oracle.  TEST INFRASTRUCTURE.

Every released number is a pure function of (stream seed, partition, slot),
so it is computed here sample by sample: Philox4x32-10 in Python integers,
uniforms and lattice arithmetic in `fractions.Fraction`, the transcendental
functions in `mpmath` at 256 bits.  Nothing is rounded before the one
rounding the kernel's final add makes:

    u         = (2 w + 1) / 2^54, w the top 53 bits of two Philox words
    g         = the smallest power of two >= scale * 2^-40 (from math.frexp)
    snap      = round(x / g), ties to even
    Laplace   k = floor(-ln(u1) b / g) - floor(-ln(u2) b / g)
    Gaussian  k = nearest integer of sigma sqrt(-2 ln u1) cos(2 pi u2) / g
    value     = float((snap + k) g)

Samples come back with their lattice index snap + k, so that a test can state
a difference in granules.  `metrics` restates the MEAN / VARIANCE / scalar
post-processing and `keep` the four selection strategies.
"""
import math
from fractions import Fraction

import mpmath
from mpmath.libmp import to_fixed

# include/dpg.h
TAG_SELECT = 0x53454C45
TAG_NOISE = 0x4E4F4953
NOISE_NONE, NOISE_LAPLACE, NOISE_GAUSSIAN = 0, 1, 2
FAMILY_SCALAR, FAMILY_MEAN, FAMILY_VARIANCE = 0, 1, 2
SLOT_COUNT, SLOT_SUM, SLOT_NSQ, SLOT_PID = 0, 1, 2, 3
V_COUNT, V_SUM, V_MEAN, V_VARIANCE, V_PRIVACY_ID_COUNT = 0, 1, 2, 3, 4
SELECT_NONE, SELECT_TRUNCATED_GEOMETRIC, SELECT_LAPLACE, SELECT_GAUSSIAN = 0, 1, 2, 3

PREC = 256  # bits of every mpmath evaluation (>= 200)
_mp = mpmath.mp.clone()  # a context of its own: the global precision stays as it is
_mp.prec = PREC
_HALF = _mp.mpf(0.5)
_M32 = 0xFFFFFFFF
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------ streams
def _mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def stream_seed(seed, nonce):
    """dpg_stream_seed: mix64(seed ^ mix64(nonce + 0x9E3779B97F4A7C15))."""
    return _mix64((seed & _M64) ^ _mix64((nonce + 0x9E3779B97F4A7C15) & _M64))


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return [c0, c1, c2, c3]


def noise_words(sseed, pk, slot):
    """The four Philox words of metric noise at (global partition, slot)."""
    pk &= _M64
    return philox4x32_10([pk & _M32, pk >> 32, slot, 0],
                         [sseed & _M32, ((sseed >> 32) & _M32) ^ TAG_NOISE])


def select_words(sseed, pk):
    pk &= _M64
    return philox4x32_10([pk & _M32, pk >> 32, 0, 0],
                         [sseed & _M32, ((sseed >> 32) & _M32) ^ TAG_SELECT])


def u53(a, b):
    """The uniform of two words: the midpoint of cell w of 2^53, exactly."""
    w = ((a << 32) | b) >> 11
    return Fraction(2 * w + 1, 1 << 54)


def u53_double(a, b):
    """The same uniform as the kernel holds it: (double(w) + 0.5) * 2^-53 in
    float64 (w + 0.5 rounds to even for w >= 2^52).  The keep table is
    compared with this double."""
    w = ((a << 32) | b) >> 11
    return (float(w) + 0.5) * 2.0 ** -53


# ------------------------------------------------------------------ lattice
def granule_exponent(scale):
    """e with 2^e the smallest power of two >= scale * 2^-40."""
    m, e = math.frexp(scale)  # scale = m 2^e, 0.5 <= m < 1
    return (e - 1 if m == 0.5 else e) - 40


def granularity(scale):
    return Fraction(2) ** granule_exponent(scale)


def snap_index(x, g):
    return round(Fraction(x) / g)  # ties to even, as rint


def _floor_checked(t):
    """floor(t), from the fixed-point integer floor(t 2^128): the 256-bit t
    decides it unless it lies within 2^-100 of an integer."""
    T = to_fixed(t._mpf_, 128)
    n = T >> 128
    frac = T - (n << 128)
    assert (1 << 28) < frac < (1 << 128) - (1 << 28), "floor undecided"
    return n


def _ln_u(u):
    """ln of the uniform (2 w + 1) / 2^54."""
    return _mp.log(_mp.mpf(u.numerator)) - _mp.log(_mp.mpf(u.denominator))


def laplace_index(b, words, g):
    """floor(-ln(u1) b / g) - floor(-ln(u2) b / g)."""
    bg = _mpf(Fraction(b) / g)
    e1 = -_ln_u(u53(words[0], words[1]))
    e2 = -_ln_u(u53(words[2], words[3]))
    return _floor_checked(e1 * bg) - _floor_checked(e2 * bg)


def gaussian_index(sigma, words, g):
    """The nearest integer of sigma sqrt(-2 ln u1) cos(2 pi u2) / g."""
    sg = _mpf(Fraction(sigma) / g)
    u2 = u53(words[2], words[3])
    r = _mp.sqrt(-2 * _ln_u(u53(words[0], words[1])))
    c = _mp.cospi(_mpf(2 * u2))
    return _floor_checked(sg * r * c + _HALF)  # a tie would fail the check


def noised(kind, x, scale, words):
    """(value as float64, lattice index, granule) of x + noise; a scale that
    is not positive, or NOISE_NONE, passes x through: (x, None, None)."""
    if kind == NOISE_NONE or not scale > 0:
        return float(x), None, None
    g = granularity(scale)
    k = (gaussian_index if kind == NOISE_GAUSSIAN else laplace_index)(scale, words, g)
    n = snap_index(x, g) + k
    return float(n * g), n, g


def noise_sample(kind, x, scale, sseed, pk, slot):
    """add_noise of the kernel: (value, lattice index)."""
    v, n, _ = noised(kind, x, scale, noise_words(sseed, pk, slot))
    return v, n


def index_offset(value, n, g, bound):
    """The d of smallest magnitude, |d| <= bound, for which the lattice point
    n + d rounds to `value` (float((n + d) g) == value), or None.  0 means
    bit-equal to the reference; where a float64 ulp exceeds the granule,
    neighbouring indices share a double and still give 0."""
    for d in sorted(range(-bound, bound + 1), key=abs):
        if float((n + d) * g) == value:
            return d
    return None


def on_lattice(value, g):
    """value / g is an integer."""
    return (Fraction(value) / g).denominator == 1


def exact(v, n, g):
    """The noised slot as an exact rational (the float itself off lattice)."""
    return Fraction(v) if n is None else n * g


# ------------------------------------------------------------------ metrics
def _mpf(q):
    """A rational as a PREC-bit mpmath number (exact for a dyadic one)."""
    return _mp.mpf(q.numerator) / q.denominator


def metrics(z, sseed, gk, cnt, sum_, nsum, nsq, rows, offsets=None):
    """The value vector V[0..4] of one kept partition (k_select_noise, the
    post-processing after the draws) as mpmath numbers at PREC bits, from the
    exact noised slots, and the lattice index of every slot drawn:
    (V, {slot: index}).  z: the dpg_noise_params fields as a dict.  offsets
    ({slot: d}) moves a slot's index by d granules: what the outputs would be
    had a sampler rounded to a neighbouring lattice point."""
    kind, scale, mask = z["noise_kind"], z["scale"], z["slot_mask"]
    idx = {}

    def draw(slot, x):
        v, n, g = noised(kind, x, scale[slot], noise_words(sseed, gk, slot))
        if n is not None and offsets:
            n += offsets.get(slot, 0)
        idx[slot] = n
        return _mpf(exact(v, n, g))

    V = [_mp.mpf(0)] * 5
    one = _mp.mpf(1)
    if z["family"] == FAMILY_VARIANCE:
        dc = draw(SLOT_COUNT, float(cnt))
        den = dc if dc > 1 else one
        mean = (_mp.mpf(z["mean_const_value"]) if z["mean_const"]
                else draw(SLOT_SUM, nsum) / den)
        msq = (_mp.mpf(z["msq_const_value"]) if z["msq_const"]
               else draw(SLOT_NSQ, nsq) / den)
        V[V_VARIANCE] = msq - mean * mean
        if not z["mean_const"]:
            mean = mean + _mp.mpf(z["mid"])
        V[V_COUNT], V[V_SUM], V[V_MEAN] = dc, mean * dc, mean
    elif z["family"] == FAMILY_MEAN:
        dc = draw(SLOT_COUNT, float(cnt))
        dn = draw(SLOT_SUM, nsum)
        mean = _mp.mpf(z["mid"]) + dn / (dc if dc > 1 else one)
        V[V_COUNT], V[V_SUM], V[V_MEAN] = dc, mean * dc, mean
    else:
        if mask & (1 << SLOT_COUNT):
            V[V_COUNT] = draw(SLOT_COUNT, float(cnt))
        if mask & (1 << SLOT_SUM):
            V[V_SUM] = draw(SLOT_SUM, sum_)
    if mask & (1 << SLOT_PID):
        V[V_PRIVACY_ID_COUNT] = draw(SLOT_PID, float(rows))
    return V, idx


def to_float(v):
    """An mpmath number rounded once to float64 (through the exact rational:
    Fraction's conversion rounds to nearest, ties to even)."""
    sign, man, exp, _ = v._mpf_
    q = Fraction(int(man)) * Fraction(2) ** exp
    return float(-q if sign else q)


# ---------------------------------------------------------------- selection
def selection_count(rows, max_rows=1, pre_threshold=0):
    """The privacy-id count the strategy sees, or None for a partition that
    is dropped before any draw: ceil(rows / max_rows), then the pre-threshold
    shift n - pre + 1."""
    if rows <= 0:
        return None
    n = -((-rows) // max_rows)
    if pre_threshold > 0:
        if n < pre_threshold:
            return None
        n = n - pre_threshold + 1
    return n


def keep(strategy, sseed, gk, rows, *, table=None, threshold=0.0, noise_scale=0.0,
         max_rows=1, pre_threshold=0, public=True):
    """(keep decision, margin): the margin of a thresholding decision is the
    exact distance of the noised count from the threshold in granules (None
    elsewhere), so a test can set aside the decisions a one-granule
    difference of the device's sample could turn."""
    if strategy == SELECT_NONE:
        return bool(public), None
    n = selection_count(rows, max_rows, pre_threshold)
    if n is None:
        return False, None
    words = select_words(sseed, gk)
    if strategy == SELECT_TRUNCATED_GEOMETRIC:
        pr = table[n] if n < len(table) else 1.0
        return u53_double(words[0], words[1]) < pr, None
    kind = NOISE_LAPLACE if strategy == SELECT_LAPLACE else NOISE_GAUSSIAN
    v, idx, g = noised(kind, float(n), noise_scale, words)
    if idx is None:
        return v > threshold, None
    d = idx * g - Fraction(threshold)
    return d > 0, abs(d) / g


# ------------------------------------------------- cases shared by the tests
# A sample may differ from this reference by one granule per rounding of a
# transcendental result (Laplace floors twice, Gaussian rounds once), and on at
# most MAX_SHARE of a case's samples (tests/test_noise_ref_cpu.py derives it).
BOUND = {NOISE_LAPLACE: 2, NOISE_GAUSSIAN: 1}
MAX_SHARE = 0.005


def step_ulps(x, ulps):
    for _ in range(abs(ulps)):
        x = math.nextafter(x, math.inf if ulps > 0 else -math.inf)
    return x


# small, fractional, powers of two and their neighbours 1 and 4 ulp away on
# both sides (where a logarithm rounds to the integer), large
SCALES = ([2.0 ** -20, 0.1, 0.75, 1.0, 3.7, 17.1826171875, 2.0 ** 30, 1e12] +
          [step_ulps(p, d) for p in (1.0, 1024.0) for d in (-4, -1, 1, 4)])


def values_for(scale):
    """Inputs on and off the lattice of `scale`: zero, a negative, a value
    with many fraction bits, rint ties (m + 1/2) g with m even and odd, and
    an integer above 2^52 (whose ulp exceeds most granules)."""
    g = float(granularity(scale))
    return [0.0, -3.25, 12345.678, 6.5 * g, 7.5 * g, -(2.0 ** 20 + 0.5) * g,
            -(2.0 ** 20 + 1.5) * g, 2.0 ** 52 + 1.0]
