"""Device columns that are not fresh, contiguous, 16-byte-aligned tensors:
a column of a [n, 3] table, every second element, buf[1:] (base address 8 mod
16: `base8`) and narrow dtypes, through DPEngine and through the C ABI.  The
columns are built on the GPU, so no host-to-device copy repairs the layout.

The reference is never the code under test: every release is compared with
the CPU oracle (or the numpy restatement the neighbouring test file uses) run
on np.ascontiguousarray copies of the same data, under those files'
tolerances: rows, count, kept sets and integer sums exactly, float sums at
rtol = atol = 1e-9.

What runs where (csrc/dpg_partition.h; one level-1 histogram group is
kScatThreads * DPG_IPT_L1 * n_cu / 8 = 360 448 records on 256 CUs, one scatter
sub-tile 11 264, and level 1 goes histogram-free from 2^22 records on):
  n = 100 001   one k_hist group, nine scatter sub-tiles, an odd last record;
  n = 720 897   three k_hist groups, the last of one record;
  n = 2^22 + 1  the piece level 1: SrcSoAKey::fetch2 loads pairs of the
                caller's columns, the last sub-tile holds one record.
SrcSoAKey::pairs_ok() is false -- k_hist's one-record loop runs -- when pid is
base8, or when a public mask is set and pk is base8; fetch2 at a base8 column
loads every pair from an address that is 8 mod 16."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from oracle import hist_oracle
from oracle import oracle
from pipelinedp_amd import analysis
from tests import layouts
from tests import percentile_ref
from tests import vector_ref
from tests import test_gpu_histograms as hist_tests
from tests import test_gpu_parity as parity
from tests import test_gpu_preaggregate as pre_tests
from tests import test_gpu_shard as shard_tests

pytestmark = pytest.mark.gpu

SEED, NONCE = parity.SEED, 0xA11C0DE
N, N_PID, P = 100_001, 8_000, 3_000
N_GROUPS = 2 * 360_448 + 1
N_PIECES = (1 << 22) + 1
EX = pdp.DataExtractors("pid", "pk", "value")
MODES = {name: kw for name, kw in parity.MODES if name in ("cross_and_per", "mean_var", "per_pid")}
ENGINE_LAYOUTS = ("column", "step2", "base8", "narrow")


def dev_view(a, layout):
    """`a` on the GPU under `layout`; base8 really is 8 mod 16."""
    if layout == "narrow":  # int32 keys, float32 values
        t = torch.from_numpy(a.astype(np.float32 if a.dtype.kind == "f" else np.int32)).cuda()
    else:
        t = layouts.torch_view(a, layout, "cuda")
    if layout == "base8":
        assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    elif layout in ("column", "step2"):
        assert not t.is_contiguous()
    return t


def base8(a):
    return dev_view(np.ascontiguousarray(a), "base8")


def aligned(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


@pytest.fixture(scope="module")
def data():
    """Zipf keys over P partitions, about 8000 privacy ids, an odd record
    count; shared and never written to."""
    return parity._dataset(11, N, N_PID, P)


def _release(cols, params, public, noise=False, backend_kw=None, select=False, **colkw):
    backend = pdp.MI355XBackend(device=0, seed=SEED, **(backend_kw or {}))
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    eng = pdp.DPEngine(acc, backend)
    col = pdp.ColumnarData(**cols, **colkw)
    if select:
        res = eng.select_partitions(col, params, pdp.DataExtractors("pid", "pk"))
    else:
        res = eng.aggregate(col, params, EX, public_partitions=public)
    acc.compute_budgets()
    res.noise_enabled = noise
    res.nonce = NONCE
    return res, res.materialize()


def _assert_partials(res, ref):
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in res.last_partials.items()}
    assert np.array_equal(got["rows"], ref["rows"])
    assert np.array_equal(got["count"], ref["count"])
    for k in ("sum", "nsum", "nsq"):
        if got[k] is not None:
            assert np.allclose(got[k], ref[k], rtol=1e-9, atol=1e-9), k


# ------------------------------------------------------------------ engine
_REFS = {}


def _oracle_ref(mode, narrow_value, data, res):
    """The oracle's partials of one mode, computed once from the first
    release's bounding fields; every later release must use the same."""
    pid, pk, val = data
    if narrow_value:  # what a float32 column holds
        val = val.astype(np.float32).astype(np.float64)
    key = (mode, narrow_value)
    if key not in _REFS:
        f = dict(res.last_bound_fields)
        ref = oracle.bound_aggregate(pid, pk, val if res.plan.needs_values() else None, f, SEED,
                                     public_mask=oracle.bitmap(range(P), P))
        _REFS[key] = (f, ref)
    f, ref = _REFS[key]
    assert res.last_bound_fields == f
    return ref


@pytest.mark.parametrize("layout", ENGINE_LAYOUTS)
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_modes_by_layout(built, data, mode, layout):
    """One column at a time, then all three.  A base8 pid takes k_hist's
    one-record loop (pairs_ok() false); public partitions = all sets no mask,
    so a base8 pk alone keeps the pair loop over pid."""
    names = ("pid", "pk", "value")
    plain = dict(zip(names, (aligned(a) for a in data)))
    odd = dict(zip(names, (dev_view(a, layout) for a in data)))
    params = pdp.AggregateParams(**MODES[mode])
    for which in names + ("all",):
        cols = {k: odd[k] if which in (k, "all") else plain[k] for k in names}
        res, _ = _release(cols, params, list(range(P)), n_partitions=P)
        ref = _oracle_ref(mode, layout == "narrow" and which in ("value", "all"), data, res)
        _assert_partials(res, ref)
    assert ref["count"].sum() < N  # the bounds bind


def test_engine_column_vector_value(built, data):
    """A scalar-metric value column of shape [n, 1]: table[:, 1:2] of a
    [n, 3] table, flattened by the ingest."""
    pid, pk, val = data
    junk = val[::-1] + 1000.0
    table = torch.from_numpy(np.stack([junk, val, junk], axis=1)).cuda()
    value = table[:, 1:2]
    assert tuple(value.shape) == (N, 1) and value.stride(0) == 3
    cols = dict(pid=aligned(pid), pk=aligned(pk), value=value)
    res, _ = _release(cols, pdp.AggregateParams(**MODES["cross_and_per"]), list(range(P)),
                      n_partitions=P)
    _assert_partials(res, _oracle_ref("cross_and_per", False, data, res))


def test_engine_private_selection_and_noise(built, data):
    """Private selection and Laplace noise at a fixed nonce: the kept set
    equals the oracle's exactly, the values to the noise granule
    (test_gpu_parity.test_gpu_selection_and_noise_match_oracle)."""
    pid, pk, val = data
    cols = dict(pid=base8(pid), pk=base8(pk), value=dev_view(val, "column"))
    params = pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        max_partitions_contributed=2, max_contributions_per_partition=1,
        min_value=0.0, max_value=10.0)
    res, out = _release(cols, params, None, noise=True, n_partitions=P)
    ref = oracle.bound_aggregate(pid, pk, val, res.last_bound_fields, SEED)
    _assert_partials(res, ref)
    keep, o = oracle.select_and_noise(ref, res.last_select_fields, res.plan.noise_fields(True),
                                      SEED, keep_table=res._table)
    ids = np.nonzero(keep)[0]
    assert 0 < len(ids) < P
    got = out.partition_ids.cpu().numpy()
    order = np.argsort(got)
    assert np.array_equal(got[order], ids)
    assert np.allclose(out.values.cpu().numpy()[order], o[ids], rtol=1e-12, atol=1e-6)


def test_engine_select_partitions_base8_keys(built, data):
    pid, pk, _ = data
    params = pdp.SelectPartitionsParams(max_partitions_contributed=3)
    res, out = _release(dict(pid=base8(pid), pk=base8(pk)), params, None, select=True,
                        n_partitions=P)
    ref = oracle.bound_aggregate(pid, pk, None, res.last_bound_fields, SEED)
    assert np.array_equal(res.last_partials["rows"].cpu().numpy(), ref["rows"])
    keep, _ = oracle.select_and_noise(ref, res.last_select_fields, parity._NO_NOISE, SEED,
                                      keep_table=getattr(res, "_table", None))
    want = np.nonzero(keep)[0]
    assert 0 < len(want) < P
    assert np.array_equal(np.sort(out.partition_ids.cpu().numpy()), want)


@pytest.fixture(scope="module")
def small():
    """20 001 records over 50 partitions (the sizes of the percentile and
    vector engine tests, whose per-record references are Python loops)."""
    rng = np.random.default_rng(23)
    n = 20_001
    pid = rng.integers(0, 2_000, n).astype(np.int64)
    pk = ((rng.zipf(1.3, n) - 1) % 50).astype(np.int64)
    return pid, pk, rng.uniform(-4.0, 68.0, n), rng.integers(-3, 14, (n, 18)).astype(np.float64)


@pytest.mark.parametrize("layout", ["column", "base8"])
def test_engine_percentiles(built, small, layout):
    """dpg_bound_records and dpg_quantile_keys read the caller's columns."""
    pid, pk, val, _ = small
    lo, hi, Ps = 0.0, 64.0, 50
    params = pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50), pdp.Metrics.PERCENTILE(90)],
        max_partitions_contributed=3, max_contributions_per_partition=2, min_value=lo,
        max_value=hi)
    cols = dict(pid=base8(pid), pk=base8(pk), value=dev_view(val, layout))
    res, out = _release(cols, params, list(range(Ps)), backend_kw=dict(percentiles=True),
                        n_partitions=Ps)
    keep = percentile_ref.kept_records(pid, pk, res.last_bound_fields, SEED, range(Ps))
    assert np.array_equal(res.last_record_keep.cpu().numpy(), keep)
    ids = out.partition_ids.cpu().numpy()
    vals = out.values.cpu().numpy()
    assert sorted(ids.tolist()) == list(range(Ps))
    assert np.array_equal(vals[:, 0], np.bincount(pk[keep == 1], minlength=Ps)[ids])
    for k, row in zip(ids.tolist(), vals[:, 1:]):
        want, margin = percentile_ref.quantiles(val[(pk == k) & (keep == 1)], [0.5, 0.9], lo, hi)
        assert margin >= 1e-9
        assert np.abs(row - want).max() <= 1e-12 * (hi - lo), (k, row, want)


@pytest.mark.parametrize("D", [3, 16])
def test_engine_vector_sum_rows_of_a_wider_table(built, small, D):
    """[n, D] rows taken as wide[:, 1:1 + D] of a [n, D + 2] table; integer
    rows, so the sums are exact."""
    pid, pk, _, table = small
    Ps = 50
    wide = torch.from_numpy(np.ascontiguousarray(table[:, :D + 2])).cuda()
    value = wide[:, 1:1 + D]
    assert not value.is_contiguous()
    rows = np.ascontiguousarray(table[:, 1:1 + D])
    params = pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.VECTOR_SUM], max_partitions_contributed=3,
        max_contributions_per_partition=2, vector_size=D, vector_max_norm=1e9,
        vector_norm_kind=pdp.NormKind.Linf)
    res, out = _release(dict(pid=base8(pid), pk=base8(pk), value=value), params,
                        list(range(Ps)), backend_kw=dict(vector_sums=True), n_partitions=Ps)
    keep = vector_ref.kept_records(pid, pk, res.last_bound_fields, SEED, range(Ps))
    assert np.array_equal(res.last_record_keep.cpu().numpy(), keep)
    want = vector_ref.partition_sums(pk, rows, keep, Ps)
    assert np.array_equal(res.last_vector_sums.cpu().numpy(), want)
    ids = out.partition_ids.cpu().numpy()
    assert np.array_equal(out.values.cpu().numpy()[:, 1:], want[ids])
    assert np.abs(want).sum() > 0


def test_analysis_preaggregate(built):
    """dpg_preaggregate sums every record's value: a strided value column."""
    rows, want = pre_tests.dataset()
    pid, pk, val = (np.array(c) for c in zip(*rows))
    cols = pdp.ColumnarData(pid=base8(pid), pk=base8(pk), value=dev_view(val, "step2"))
    got = list(analysis.preaggregate(cols, pre_tests._backend(), EX))
    assert len(got) == sum(len(v) for v in want.values())
    pre_tests._assert_rows_match(got, want)


def test_public_partitions_summary_base8_keys(built):
    from pipelinedp_amd.analysis import dataset_summary
    rng = np.random.default_rng(33)
    n, Pn = 200_001, 100_003
    pk = rng.integers(0, Pn, n)
    pk[:5] = [0, 7, 8, Pn - 2, Pn - 1]
    pub = np.arange(1_000, 90_001)
    cols = pdp.ColumnarData(pk=base8(pk), n_partitions=Pn)
    (s,) = list(dataset_summary.compute_public_partitions_summary(
        cols, pre_tests._backend(), pdp.DataExtractors(partition_extractor="pk"),
        range(1_000, 90_001)))
    present = np.unique(pk)
    both = len(np.intersect1d(present, pub))
    assert (s.num_dataset_public_partitions, s.num_dataset_non_public_partitions,
            s.num_empty_public_partitions) == (both, len(present) - both, len(pub) - both)
    assert 0 < both < len(present) and both < len(pub)


def test_dataset_histograms(built, data):
    from pipelinedp_amd.dataset_histograms import computing_histograms as ch
    pid, pk, val = data
    cols = pdp.ColumnarData(pid=base8(pid), pk=base8(pk), value=dev_view(val, "column"))
    (hs,) = list(ch.compute_dataset_histograms(cols, hist_tests.EXC,
                                               pdp.MI355XBackend(device=0, seed=9)))
    hist_tests.assert_same(hist_tests.plain(hs), hist_oracle.dataset_histograms(pid, pk, val),
                           "layouts")


def test_engine_sparse_partition_keys_base8(built, data):
    """dpg_keydict_insert reads the caller's pk: any int64 keys, base8."""
    pid, pk, val = data
    keys = pk * 1_000_003 - 1_500_000_001
    uniq, dense = np.unique(keys, return_inverse=True)
    params = pdp.AggregateParams(**MODES["cross_and_per"])
    cols = dict(pid=aligned(pid), pk=base8(keys), value=dev_view(val, "column"))
    res, out = _release(cols, params, torch.from_numpy(uniq), sparse_partition_keys=True)
    assert np.array_equal(res.last_key_dictionary.ids.cpu().numpy(), dense)
    f = res.last_bound_fields
    assert f["n_partitions"] == len(uniq)
    ref = oracle.bound_aggregate(pid, dense.astype(np.int64), val, f, SEED,
                                 public_mask=oracle.bitmap(range(len(uniq)), len(uniq)))
    _assert_partials(res, ref)
    got = out.partition_ids.cpu().numpy()   # the caller's keys
    order = np.argsort(got)
    assert np.array_equal(got[order], uniq)
    assert np.array_equal(out.values.cpu().numpy()[order, 0], ref["count"].astype(np.float64))


def test_engine_wide_privacy_ids_base8(built, data):
    """dpg_keydict_insert_slots reads the caller's pid: ids spread over 2^63."""
    pid, pk, val = data
    rng = np.random.default_rng(2025)
    pool = np.unique(rng.integers(-(1 << 62), 1 << 62, N_PID + 100, dtype=np.int64))[:N_PID]
    rng.shuffle(pool)
    wide = pool[pid]
    uniq, ranked = np.unique(wide, return_inverse=True)
    params = pdp.AggregateParams(**MODES["cross_and_per"])
    cols = dict(pid=base8(wide), pk=aligned(pk), value=dev_view(val, "step2"))
    res, _ = _release(cols, params, list(range(P)), n_partitions=P, wide_privacy_ids=True)
    f = res.last_bound_fields
    assert (f["pid_min"], f["pid_count"]) == (0, len(uniq))
    ref = oracle.bound_aggregate(ranked.astype(np.int64), pk, val, f, SEED,
                                 public_mask=oracle.bitmap(range(P), P))
    _assert_partials(res, ref)


# ------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, SEED)
    yield c
    c.close()


PUBLIC = range(0, P, 2)


def _fields(**kw):
    f = dict(mode=percentile_ref.MODE_CROSS_AND_PER, sum_mode=1, metric_mask=3,
             max_partitions_contributed=3, max_contributions_per_partition=2, max_contributions=0,
             min_value=0.0, max_value=10.0, min_sum_per_partition=0.0, max_sum_per_partition=0.0,
             n_partitions=P, pid_min=0, pid_count=0, rec_id_offset=0, nonce=99)
    f.update(kw)
    return f


def _int_records(n, n_pid):
    """Integer values: the clipped sums are exact in any order, so two calls
    can be compared bit for bit."""
    pid, pk, _ = parity._dataset(17, n, n_pid, P)
    val = np.random.default_rng(18).integers(-3, 14, n).astype(np.float64)
    return pid, pk, val


def _abi_bound_aggregate(ctx, d_pid, d_pk, d_val, n, f, d_mask):
    from pipelinedp_amd import _native
    bound = _native.fill(_native.BoundParams, f)
    bound.public_mask = d_mask.data_ptr()
    rows, count = (torch.full((P,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    sums = torch.full((P,), -7.0, dtype=torch.float64, device="cuda")
    partials = _native.Partials(P, rows.data_ptr(), count.data_ptr(), sums.data_ptr(), None, None)
    ctx.bound_aggregate(d_pid.data_ptr(), d_pk.data_ptr(), d_val.data_ptr(), n, bound, partials,
                        None)
    torch.cuda.synchronize()
    return dict(rows=rows.cpu().numpy(), count=count.cpu().numpy(), sum=sums.cpu().numpy())


def _check_bound_aggregate(ctx, n, n_pid, combos, stage):
    pid, pk, val = _int_records(n, n_pid)
    f = _fields()
    mask = oracle.bitmap(PUBLIC, P)
    ref = oracle.bound_aggregate(pid, pk, val, f, SEED, public_mask=mask)
    assert 0 < ref["count"].sum() < n
    d_mask = torch.from_numpy(mask).cuda()
    plain = _abi_bound_aggregate(ctx, aligned(pid), aligned(pk), aligned(val), n, f, d_mask)
    for odd in combos:
        cols = [base8(a) if name in odd else aligned(a)
                for name, a in (("pid", pid), ("pk", pk), ("value", val))]
        got = _abi_bound_aggregate(ctx, *cols, n, f, d_mask)
        assert any(stage in s for s in ctx.stage_times()), ctx.stage_times()
        for k in ("rows", "count", "sum"):
            assert np.array_equal(got[k], ref[k]), (odd, k)
            assert np.array_equal(got[k], plain[k]), (odd, k)


def test_abi_bound_aggregate_base8(ctx):
    """With a public mask pairs_ok() has two operands: every column base8,
    pid alone (first operand false), pk alone (second operand false): k_hist's
    one-record loop each time; the scatter loads single records (an odd
    DPG_IPT_L1)."""
    _check_bound_aggregate(ctx, N, N_PID, (("pid", "pk", "value"), ("pid",), ("pk",)),
                           "partition1:hist")


def test_abi_bound_aggregate_base8_three_hist_groups(ctx):
    """Three k_hist groups, the last of one record."""
    _check_bound_aggregate(ctx, N_GROUPS, 60_000, (("pid", "pk", "value"),), "partition1:hist")


def test_abi_bound_aggregate_base8_piece_level(ctx):
    """The histogram-free level 1: fetch2 loads two records of each caller
    column at once, every pair at an address 8 mod 16; the last sub-tile
    holds one record and loads the pair that ends with it."""
    _check_bound_aggregate(ctx, N_PIECES, 350_000, (("pid", "pk", "value"), ("pk",)),
                           "partition1:pieces")


def test_abi_bound_records_base8(ctx):
    from pipelinedp_amd import _native
    n = 5_001
    pid, pk, val = _int_records(n, 300)
    f = _fields()
    bound = _native.fill(_native.BoundParams, f)
    d_mask = torch.from_numpy(oracle.bitmap(PUBLIC, P)).cuda()
    bound.public_mask = d_mask.data_ptr()
    want = percentile_ref.kept_records(pid, pk, f, SEED, PUBLIC)
    assert 0 < want.sum() < n
    for odd in ((), ("pid", "pk"), ("pid",), ("pk",)):
        d_pid = base8(pid) if "pid" in odd else aligned(pid)
        d_pk = base8(pk) if "pk" in odd else aligned(pk)
        keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        ctx.bound_records(d_pid.data_ptr(), d_pk.data_ptr(), n, bound, keep.data_ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(keep.cpu().numpy(), want), odd


def test_abi_check_shard_base8(ctx):
    pid, _, _ = _int_records(N, N_PID)
    pid = pid * 0x1_0000_0001 - (1 << 40)   # ids of either sign, above 2^32
    n_bad = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for world, rank in ((2, 1), (3, 0), (8, 5)):
        want = int((shard_tests._shard_np(pid, world) != rank).sum())
        assert 0 < want < N
        for d_pid in (aligned(pid), base8(pid)):
            ctx.check_shard(d_pid.data_ptr(), N, world, rank, n_bad.data_ptr(), None)
            assert int(n_bad.item()) == want


def test_abi_keydict_insert_base8(ctx):
    i64_min = -(1 << 63)
    rng = np.random.default_rng(5)
    pool = rng.integers(i64_min + 1, (1 << 63) - 1, 5_000, dtype=np.int64)
    keys = pool[rng.integers(0, len(pool), N)]
    keys[7] = i64_min                        # the reserved key is counted, not inserted
    want = np.unique(keys[keys != i64_min])
    cap = 16_384
    for d_keys in (aligned(keys), base8(keys)):
        slots = torch.full((cap,), i64_min, dtype=torch.int64, device="cuda")
        info = torch.zeros(2, dtype=torch.int64, device="cuda")
        ctx.keydict_insert(d_keys.data_ptr(), N, slots.data_ptr(), cap, info.data_ptr(), None)
        out = torch.full((cap,), 12345, dtype=torch.int64, device="cuda")
        cnt = torch.full((1,), -9, dtype=torch.int64, device="cuda")
        ctx.keydict_keys(slots.data_ptr(), cap, out.data_ptr(), cnt.data_ptr(), None)
        assert info.tolist() == [1, 0]
        assert np.array_equal(np.sort(out[:int(cnt.item())].cpu().numpy()), want)


def test_abi_sample_partitions_base8(ctx):
    """keys must be 8-byte aligned (dpg_api.hip): base8 is."""
    from pipelinedp_amd.analysis import utility_analysis as ua_mod
    n = 2_001
    keys = np.random.default_rng(6).integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    bound = ua_mod._sample_bound(0.5)
    sha = [int(hashlib.sha1(repr(int(k)).encode()).hexdigest()[:16], 16) for k in keys]
    want = np.zeros(8 * ((n + 63) // 64), np.uint8)
    packed = np.packbits(np.array([h < bound for h in sha], bool), bitorder="little")
    want[:len(packed)] = packed
    for d_keys in (aligned(keys), base8(keys)):
        mask = torch.full((len(want),), 0xFF, dtype=torch.uint8, device="cuda")
        hashes = torch.zeros(n, dtype=torch.int64, device="cuda")
        ctx.sample_partitions(ctypes.c_void_p(d_keys.data_ptr()), 0, 1, n, bound,
                              ctypes.c_void_p(mask.data_ptr()),
                              ctypes.c_void_p(hashes.data_ptr()), None)
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want)
        assert hashes.cpu().numpy().view(np.uint64).tolist() == sha
