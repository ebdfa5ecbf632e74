"""k_select_noise (through dpg_select_and_noise, hand-made partials) against
the exact reference of tests/noise_ref.py, sample by sample and decision by
decision.

Every noised output must lie on the exact lattice of its scale.  Its index
may differ from the reference's by one granule per rounding of a
transcendental result (|d| <= 2 for Laplace, <= 1 for Gaussian) on at most
0.5 % of a case's samples; every other sample is bit-equal.  Keep decisions
equal the reference's; only a thresholding decision whose exact noised count
lies within 2 granules of the threshold is set aside.

The arms reached: the keep table in LDS and in global memory, pk_offset /
pk_stride with keys above 2^32, max_rows_per_privacy_id with a pre-threshold,
the denominator clamp of MEAN / VARIANCE with negative noised counts,
mean_const / msq_const, an out_src map of 8 columns, the public mask, and the
grid-stride loop."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import noise_ref as nr
from tests.noise_ref import BOUND, MAX_SHARE, SCALES, values_for

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F5E1EC7
NONCE = 0xC0FFEE
DEV = "cuda:0"
KINDS = pytest.mark.parametrize("kind", [nr.NOISE_LAPLACE, nr.NOISE_GAUSSIAN],
                                ids=["laplace", "gaussian"])
_NOISE_OFF = dict(noise_kind=0, family=0, slot_mask=0, n_outputs=0, out_src=[0] * 8,
                  scale=[0.0] * 4, mid=0.0, mean_const=0, msq_const=0, mean_const_value=0.0,
                  msq_const_value=0.0)


@pytest.fixture(scope="module")
def backend(built):
    import pipelinedp_amd as pdp
    return pdp.MI355XBackend(device=0, seed=SEED)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(backend, rows, count, sum_=None, nsum=None, nsq=None, select=None, noise=None,
          table=None, mask=None):
    """One dpg_select_and_noise over hand-made partials: (keep[P], out[P, n_outputs]).
    keep and out are pre-filled with 7 and NaN, so an unwritten entry shows."""
    from pipelinedp_amd import _native
    P = len(rows)
    t = [_dev(a) for a in (np.asarray(rows, np.int64), np.asarray(count, np.int64), sum_, nsum,
                           nsq)]
    parts = _native.Partials(P, *[_ptr(x) for x in t])
    f = dict(strategy=nr.SELECT_NONE, table_len=0, keep_table=None, threshold=0.0,
             noise_scale=0.0, pre_threshold=0, max_rows_per_privacy_id=1, pk_offset=0,
             public_mask=None, nonce=NONCE, pk_stride=1)
    f.update(select or {})
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.float64)
        f["table_len"], f["keep_table"] = len(table), table.ctypes.data
    bitmap = None
    if mask is not None:
        bitmap = _dev(np.packbits(np.asarray(mask, bool), bitorder="little"))
        f["public_mask"] = bitmap.data_ptr()
    z = dict(_NOISE_OFF)
    z.update(noise or {})
    n_out = z["n_outputs"]
    keep = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
    out = torch.full((max(P * n_out, 1),), float("nan"), dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV))
    backend.ctx.select_and_noise(parts, _native.fill(_native.SelectParams, f),
                                 _native.fill(_native.NoiseParams, z), keep.data_ptr(),
                                 out.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    return keep.cpu().numpy(), out.cpu().numpy()[:P * n_out].reshape(P, n_out)


def _assert_on_lattice(column, scale):
    q = column / float(nr.granularity(scale))  # a power of two: the quotient is exact
    assert np.all(q == np.rint(q)), "an output is off the exact lattice of its scale"


def _count_differing(got, kind, xs, scale, sseed, gks, slot):
    """Checks got[i] against the reference sample at (gks[i], slot) with input
    xs[i]; returns how many lie on a neighbouring lattice point."""
    g = nr.granularity(scale)
    want = np.empty(len(got))
    differing = 0
    for i, (v, x, gk) in enumerate(zip(got, xs, gks)):
        want[i], n = nr.noise_sample(kind, float(x), scale, sseed, int(gk), slot)
        d = nr.index_offset(float(v), n, g, BOUND[kind])
        assert d is not None, (int(gk), slot, float(x), float(v), want[i])
        if d != 0:
            differing += 1
            want[i] = v
    assert np.array_equal(got, want)
    return differing


def _report(what, differing, total):
    print(f"[noise-exact] {what}: {differing} of {total} samples one granule off "
          f"({100.0 * differing / total:.3f} %)")
    assert differing <= MAX_SHARE * total, (what, differing, total)


# ------------------------------------------------------------ scalar slots
TRIPLES = [SCALES[i:i + 3] for i in (0, 3, 6, 9, 12)] + [SCALES[13:16]]
P_SCALAR = 4099  # 17 blocks of 256, the last with 3 partitions


def _scalar_inputs(sum_scale):
    rng = np.random.default_rng(3)
    special = np.array([0, 1, 2 ** 40], np.int64)
    count = rng.integers(0, 1000, P_SCALAR)
    rows = rng.integers(0, 1000, P_SCALAR)
    for at in (0, 254, P_SCALAR - 3):  # head, across a block boundary, ragged tail
        count[at:at + 3] = special
        rows[at:at + 3] = special[::-1]
    xs = values_for(sum_scale)
    sum_ = rng.normal(0.0, 100.0, P_SCALAR)
    sum_[::2] = [xs[i % len(xs)] for i in range(len(sum_[::2]))]
    return rows, count, sum_


@KINDS
@pytest.mark.parametrize("scales", TRIPLES, ids=[f"{t[0].hex()}.." for t in TRIPLES])
def test_scalar_slots_exact(backend, kind, scales):
    rows, count, sum_ = _scalar_inputs(scales[1])
    slots = (nr.SLOT_COUNT, nr.SLOT_SUM, nr.SLOT_PID)
    scale = [0.0] * 4
    for s, v in zip(slots, scales):
        scale[s] = v
    noise = dict(noise_kind=kind, family=nr.FAMILY_SCALAR, slot_mask=0b1011, n_outputs=3,
                 out_src=[nr.V_COUNT, nr.V_SUM, nr.V_PRIVACY_ID_COUNT, 0, 0, 0, 0, 0],
                 scale=scale)
    keep, out = _call(backend, rows, count, sum_=sum_, noise=noise)
    assert np.all(keep == 1)
    inputs = [count.astype(np.float64), sum_, rows.astype(np.float64)]
    # about 5000 reference samples: both ends (the ragged tail), every fourth between
    pick = np.unique(np.r_[0:320, P_SCALAR - 320:P_SCALAR, 320:P_SCALAR - 320:4])
    sseed = nr.stream_seed(SEED, NONCE)
    differing = 0
    for col, (slot, x) in enumerate(zip(slots, inputs)):
        _assert_on_lattice(out[:, col], scale[slot])
        differing += _count_differing(out[pick, col], kind, x[pick], scale[slot], sseed, pick,
                                      slot)
    _report(f"scalar kind {kind} scales {[s.hex() for s in scales]}", differing, 3 * len(pick))

    noise["noise_kind"] = nr.NOISE_NONE
    keep, out = _call(backend, rows, count, sum_=sum_, noise=noise)
    for col, x in enumerate(inputs):
        assert np.array_equal(out[:, col], x)


# ------------------------------------------------------------------ keying
@KINDS
def test_keys_above_2_32_stride_nonce_and_family(backend, kind):
    n, hi = 1000, 2 ** 32
    rng = np.random.default_rng(8)
    big = 5 + 3 * (n - 1) + 1
    count_b = rng.integers(0, 500, big)
    sum_b = rng.normal(0.0, 50.0, big)
    rows_b = np.ones(big, np.int64)
    count_a, sum_a, rows_a = count_b[5::3], sum_b[5::3], rows_b[5::3]
    assert len(count_a) == n
    scale = [3.7, 0.75, 17.1826171875, 0.0]
    noise = dict(noise_kind=kind, family=nr.FAMILY_SCALAR, slot_mask=0b0011, n_outputs=2,
                 out_src=[nr.V_COUNT, nr.V_SUM, 0, 0, 0, 0, 0, 0], scale=scale)
    strided = dict(pk_offset=hi + 5, pk_stride=3)
    _, a = _call(backend, rows_a, count_a, sum_=sum_a, noise=noise, select=strided)
    _, b = _call(backend, rows_b, count_b, sum_=sum_b, noise=noise, select=dict(pk_offset=hi))
    assert np.array_equal(a, b[5::3])

    gks = hi + 5 + 3 * np.arange(n)
    sseed = nr.stream_seed(SEED, NONCE)
    differing = _count_differing(a[:, 0], kind, count_a, scale[0], sseed, gks, nr.SLOT_COUNT)
    differing += _count_differing(a[:, 1], kind, sum_a, scale[1], sseed, gks, nr.SLOT_SUM)
    _report(f"keying kind {kind}", differing, 2 * n)
    # the high counter word matters: the same low words give other samples
    _, low = _call(backend, rows_a, count_a, sum_=sum_a, noise=noise,
                   select=dict(pk_offset=5, pk_stride=3))
    assert np.mean(low[:, 0] != a[:, 0]) > 0.99

    _, other = _call(backend, rows_a, count_a, sum_=sum_a, noise=noise,
                     select=dict(strided, nonce=NONCE + 1))
    assert np.mean(other != a) > 0.99

    # COUNT draws slot 0 whatever the family
    only_count = dict(noise, slot_mask=0, n_outputs=1, out_src=[nr.V_COUNT] + [0] * 7)
    for family in (nr.FAMILY_MEAN, nr.FAMILY_VARIANCE):
        _, c = _call(backend, rows_a, count_a, nsum=sum_a, nsq=sum_a * sum_a,
                     noise=dict(only_count, family=family), select=strided)
        assert np.array_equal(c[:, 0], a[:, 0])


# ------------------------------------------------------------- grid-stride
def test_grid_stride_loop_draws_the_reference_noise(backend):
    first_pass = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256
    P = 1_048_576 + 300
    assert P > first_pass, "the launch covers P in one pass: the loop is not reached"
    count = (np.arange(P, dtype=np.int64) * 7) % 1000
    scale = 3.7
    noise = dict(noise_kind=nr.NOISE_LAPLACE, family=nr.FAMILY_SCALAR, slot_mask=0b0001,
                 n_outputs=1, out_src=[nr.V_COUNT] + [0] * 7, scale=[scale, 0.0, 0.0, 0.0])
    keep, out = _call(backend, np.ones(P, np.int64), count, noise=noise)
    assert np.all(keep == 1)
    _assert_on_lattice(out[:, 0], scale)
    rng = np.random.default_rng(21)
    pick = np.unique(np.r_[0:512, P - 512:P, first_pass - 256:first_pass + 256,
                           rng.integers(0, P, 2000)])
    differing = _count_differing(out[pick, 0], nr.NOISE_LAPLACE, count[pick].astype(np.float64),
                                 scale, nr.stream_seed(SEED, NONCE), pick, nr.SLOT_COUNT)
    _report("grid-stride laplace", differing, len(pick))


# ------------------------------------------------------- MEAN and VARIANCE
# Inputs under which 4 ulp holds for a correctly rounded evaluation of the
# kernel's formulas against the exact one.  COUNT has scale 50 on counts in
# {0, 1, 2, 1000}: most denominators are clamped to 1 and many noised counts
# are negative.  nsum in [-3, 3] with scale 0.75 keeps |noised nsum| below 40,
# nsq in [5000, 5100] with scale 17.18 keeps noised nsq above 4000, so in
#   var = msq - mean * mean    (mean^2 / msq = dn^2 / (dq den) < 0.4)
#   mean = mid + dn / den      (mid = 100, |dn / den| < 40)
# no subtraction loses more than one bit: each output is at most four
# roundings (a quotient, a product, a sum, one more product) of half an ulp,
# the two inner ones scaled down, i.e. below 3 ulp.  The constants are chosen
# the same way: mean_const_value^2 = 0.25 against msq > 1.3 (den < 2900),
# msq_const_value = 5000 against mean^2 < 1600.  Every noised slot is a multiple of 2^-40 below
# 2^13, hence exact in float64.
P_MOMENTS = 2000
MOMENT_SCALES = [50.0, 0.75, 17.1826171875, 0.1]
OUT_SRC = [nr.V_VARIANCE, nr.V_COUNT, nr.V_PRIVACY_ID_COUNT, nr.V_MEAN, nr.V_SUM, nr.V_COUNT,
           nr.V_VARIANCE, nr.V_MEAN]
ARMS = {
    "mean": dict(family=nr.FAMILY_MEAN),
    "variance": dict(family=nr.FAMILY_VARIANCE),
    "mean_const": dict(family=nr.FAMILY_VARIANCE, mean_const=1, mean_const_value=0.5),
    "msq_const": dict(family=nr.FAMILY_VARIANCE, msq_const=1, msq_const_value=5000.0),
    "both_const": dict(family=nr.FAMILY_VARIANCE, mean_const=1, mean_const_value=0.5,
                       msq_const=1, msq_const_value=5000.0),
}


def _within_4_ulp(got, V):
    want = np.array([nr.to_float(V[s]) for s in OUT_SRC])
    return bool(np.all(np.abs(got - want) <= 4 * np.spacing(np.abs(want))))


@KINDS
@pytest.mark.parametrize("arm", list(ARMS))
def test_mean_variance_arms(backend, kind, arm):
    rng = np.random.default_rng(13)
    P = P_MOMENTS
    count = rng.choice(np.array([0, 1, 2, 1000], np.int64), P)
    rows = rng.integers(1, 50, P)
    nsum = rng.uniform(-3.0, 3.0, P)
    nsq = rng.uniform(5000.0, 5100.0, P)
    mask = rng.random(P) < 0.6  # a public mask with holes
    mask[:16] = [True, False] * 8
    z = dict(_NOISE_OFF, noise_kind=kind, slot_mask=1 << nr.SLOT_PID, n_outputs=8,
             out_src=OUT_SRC, scale=MOMENT_SCALES, mid=100.0, **ARMS[arm])
    keep, out = _call(backend, rows, count, nsum=nsum, nsq=nsq, noise=z, mask=mask)
    assert np.array_equal(keep, mask.astype(np.uint8))
    assert np.all(out[~mask] == 0.0)
    assert not np.isnan(out).any()
    for col in (1, 5):
        _assert_on_lattice(out[mask, col], MOMENT_SCALES[nr.SLOT_COUNT])
    _assert_on_lattice(out[mask, 2], MOMENT_SCALES[nr.SLOT_PID])

    sseed = nr.stream_seed(SEED, NONCE)
    bound = BOUND[kind]
    g = {s: nr.granularity(MOMENT_SCALES[s]) for s in range(4)}
    off = {s: 0 for s in range(4)}  # partitions with the slot's index a granule off
    clamped = negative = 0
    for k in np.flatnonzero(mask):
        args = (z, sseed, int(k), int(count[k]), 0.0, float(nsum[k]), float(nsq[k]), int(rows[k]))
        V, idx = nr.metrics(*args)
        clamped += V[nr.V_COUNT] <= 1
        negative += V[nr.V_COUNT] < 0
        if _within_4_ulp(out[k], V):
            continue
        # COUNT and PRIVACY_ID_COUNT are outputs: their offsets are read off;
        # those of the sum slots are the ones that explain the other outputs
        fixed = {}
        for slot, col in ((nr.SLOT_COUNT, 1), (nr.SLOT_PID, 2)):
            d = nr.index_offset(float(out[k, col]), idx[slot], g[slot], bound)
            assert d is not None, (int(k), slot, out[k].tolist())
            fixed[slot] = d
        hidden = [s for s in (nr.SLOT_SUM, nr.SLOT_NSQ) if s in idx]
        found = None
        for ds in sorted(itertools.product(range(-bound, bound + 1), repeat=len(hidden)),
                         key=lambda t: sum(map(abs, t))):
            offsets = {**fixed, **dict(zip(hidden, ds))}
            if _within_4_ulp(out[k], nr.metrics(*args, offsets=offsets)[0]):
                found = offsets
                break
        assert found is not None, (int(k), out[k].tolist(), [nr.to_float(V[s]) for s in OUT_SRC])
        for slot, d in found.items():
            off[slot] += d != 0
    kept = int(mask.sum())
    assert clamped > kept // 4 and negative > kept // 8, "the clamp is not reached"
    print(f"[noise-exact] {arm} kind {kind}: partitions a granule off per slot {off} of {kept}")
    for slot, n_off in off.items():
        assert n_off <= MAX_SHARE * kept, (arm, slot, n_off, kept)


# --------------------------------------------------------------- selection
P_SELECT = 20_000


def _plan(strategy, eps, delta, l0, pre=None):
    from pipelinedp_amd import partition_selection as ps
    from pipelinedp_amd.aggregate_params import PartitionSelectionStrategy as S
    return ps.create_partition_selection_strategy(getattr(S, strategy), eps, delta, l0, pre)


@pytest.mark.parametrize("max_rows,pre", [(1, 0), (3, 4)], ids=["plain", "max_rows3_pre4"])
@pytest.mark.parametrize("eps,top,arm", [(1e-3, 9000, "global"), (1.0, 40, "lds")],
                         ids=["table_in_global_memory", "table_in_lds"])
def test_truncated_geometric_decisions(backend, eps, top, arm, max_rows, pre):
    from pipelinedp_amd import partition_selection as ps
    plan = _plan("TRUNCATED_GEOMETRIC", eps, 1e-5, 1, pre or None)
    table = np.asarray(plan.table, np.float64)
    assert (len(table) > 4096) == (arm == "global"), len(table)
    rows = np.random.default_rng(17).integers(0, top * max_rows + 1, P_SELECT)
    rows[:4] = [0, 1, max_rows, top * max_rows]
    offset = 2 ** 32 - 7  # keys on both sides of the counter's high word
    keep, _ = _call(backend, rows, rows, table=table,
                    select=dict(strategy=nr.SELECT_TRUNCATED_GEOMETRIC, pre_threshold=pre,
                                max_rows_per_privacy_id=max_rows, pk_offset=offset))
    sseed = nr.stream_seed(SEED, NONCE)
    want = np.empty(P_SELECT, np.uint8)
    for k in range(P_SELECT):
        want[k], _ = nr.keep(nr.SELECT_TRUNCATED_GEOMETRIC, sseed, offset + k, int(rows[k]),
                             table=table, max_rows=max_rows, pre_threshold=pre)
        # the same decision from the host's own keep probability
        n = -(-int(rows[k]) // max_rows)
        u = nr.u53_double(*nr.select_words(sseed, offset + k)[:2])
        assert bool(want[k]) == (u < ps.probability_of_keep(plan, n))
    assert 0.05 < want.mean() < 0.95, "the case decides nothing"
    assert np.array_equal(keep, want)


@pytest.mark.parametrize("strategy,native", [("LAPLACE_THRESHOLDING", nr.SELECT_LAPLACE),
                                             ("GAUSSIAN_THRESHOLDING", nr.SELECT_GAUSSIAN)],
                         ids=["laplace", "gaussian"])
def test_thresholding_decisions(backend, strategy, native):
    plan = _plan(strategy, 1.0, 1e-3, 2)
    rows = np.random.default_rng(19).integers(1, 41, P_SELECT)
    keep, _ = _call(backend, rows, rows,
                    select=dict(strategy=native, threshold=plan.threshold,
                                noise_scale=plan.noise_scale))
    sseed = nr.stream_seed(SEED, NONCE)
    want = np.empty(P_SELECT, np.uint8)
    near = 0
    for k in range(P_SELECT):
        want[k], margin = nr.keep(native, sseed, k, int(rows[k]), threshold=plan.threshold,
                                  noise_scale=plan.noise_scale)
        if margin <= 2:  # a granule's difference may turn it: expected about 1e-7 of them
            near += 1
            want[k] = keep[k]
    assert near <= 5, near
    assert 0.05 < want.mean() < 0.95, "the case decides nothing"
    assert np.array_equal(keep, want)
