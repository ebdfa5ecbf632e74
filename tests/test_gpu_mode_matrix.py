"""GPU mode matrix: every bounding kernel of dpg_bound_aggregate in the
bounding modes, sum modes and item layouts that tests/test_gpu_parity.py
leaves out, on its inputs and through its forcing hooks, with exact values
(tests/exact_values.py): rows, counts and every float partial equal the
oracle's bit for bit.

Per-partition sum clipping is the one accumulator that is not additive: a
kernel that emits two items for one (privacy id, partition) pair -- across
streamed pieces, a restart, a deferral or the heavy cut -- clamps that pair's
sum twice.  With exact values no rounding can hide it, or a record swapped
for another, or a term dropped at a low magnitude.

tests/test_exact_values_cpu.py checks for every (mode, input) pair here that
sampling and clipping bind.  The release nonce is fixed, so those conditions
hold for these very runs and one oracle run serves every variant of a pair.
"""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from oracle import oracle
from pipelinedp_amd import combiners
from tests import exact_values as ev

pytestmark = pytest.mark.gpu

_HOOKS = ("DPG_BOUND_HASH", "DPG_MW_OFF", "DPG_MW_MEDIUM", "DPG_MEDIUM_STREAM", "DPG_NO_HEAVY",
          "DPG_STREAM_OVER")


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for h in _HOOKS:
        monkeypatch.delenv(h, raising=False)


_REFS = {}


def _reference(gen, fields):
    """The oracle's partials of an input under the release's bound fields;
    computed once per distinct fields (the variants of a pair share them)."""
    key = (gen, tuple(sorted(fields.items())))
    if key not in _REFS:
        pid, pk, val, P = ev.dataset(gen)
        ref = oracle.bound_aggregate(pid, pk, val, fields, ev.SEED)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _run(mode, gen, tuning=None):
    """One noise-free release of the pair; returns its stage markers after
    comparing the partials with the oracle's."""
    pid, pk, val, P = ev.dataset(gen)
    backend = pdp.MI355XBackend(device=0, seed=ev.SEED)
    if tuning is not None:
        backend.ctx.set_tuning(*tuning)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    res = pdp.DPEngine(acc, backend).aggregate(
        pdp.ColumnarData(pid=torch.from_numpy(pid.copy()), pk=torch.from_numpy(pk.copy()),
                         value=torch.from_numpy(val.copy()), n_partitions=P),
        ev.make_params(mode, gen), pdp.DataExtractors("pid", "pk", "value"),
        public_partitions=list(range(P)) if P <= 20_000 else None)
    ev.override_plan(res.plan, mode, gen)
    acc.compute_budgets()
    res.noise_enabled = False
    res.nonce = ev.NONCE
    res.materialize()
    st = backend.ctx.stage_times()
    fields = res.last_bound_fields
    _, want_mode, want_sum = ev.MODES[mode]
    assert (fields["mode"], fields["sum_mode"]) == (want_mode, want_sum)
    assert fields["nonce"] == ev.NONCE
    var = bool(fields["metric_mask"] & (combiners.M_MEAN | combiners.M_VARIANCE))
    has_sum = bool(fields["metric_mask"] & combiners.M_SUM)
    ref = _reference(gen, fields)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in res.last_partials.items()}
    assert np.array_equal(got["rows"], ref["rows"])
    assert np.array_equal(got["count"], ref["count"])
    # which partials exist says which item layout ran: Item16 (sum or
    # nothing), ItemV (nsum, nsq), Item32 (all three)
    assert (got["sum"] is not None) == has_sum
    assert (got["nsum"] is not None) == (got["nsq"] is not None) == var
    assert has_sum or var or want_sum == ev.NONE
    for k in ("sum", "nsum", "nsq"):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k]), (k, _mismatch(got[k], ref[k]))
    return st


def _mismatch(got, ref):
    bad = np.nonzero(got != ref)[0]
    return (f"{bad.size} partitions differ; first {bad[:5].tolist()}: "
            f"got {got[bad[:5]].tolist()} want {ref[bad[:5]].tolist()}")


def _modes(gen):
    return [m for m, g in ev.PAIRS if g == gen]


_SMALL = [(m, k) for m in _modes("small") for k in ("sort", "hash")
          if k == "hash" or not ev.is_per_pid(m)]


@pytest.mark.parametrize("mode,kernel", _SMALL, ids=[f"{m}-{k}" for m, k in _SMALL])
def test_small_chunk_kernels(built, monkeypatch, mode, kernel):
    """k_bound_sorted tier 0 / 1 and k_bound_waves on chunks of ~40-record
    privacy ids (test_gpu_small_chunk_kernels_match_oracle's input).  The
    PER_PRIVACY_ID modes always take the hash kernel (k_bound_waves<true>),
    so they run once; the marker says which kernel ran."""
    if kernel == "hash":
        monkeypatch.setenv("DPG_BOUND_HASH", "1")
    st = _run(mode, "small")
    assert [k for k in st if k.startswith("bound.kernel=")] == ["bound.kernel=" + kernel]


_WM = [(m, v) for m in ev.CROSS_MODES for v in ("multiwave", "default", "single", "hash_medium")]
_WM += [("perpid_sum_pp", "default"), ("perpid_var", "default")]


@pytest.mark.parametrize("mode,mw", _WM, ids=[f"{m}-{v}" for m, v in _WM])
def test_wide_and_medium_chunks(built, monkeypatch, mode, mw):
    """Wide chunks (two 200-record ids) and medium chunks (one 700-record id
    per fine bucket) of test_gpu_wide_and_medium_chunks_match_oracle: the
    2-wave wide kernel, the 4-wave medium kernel (DPG_MW_MEDIUM), the
    single-wave 8-element kernel (DPG_MW_OFF), the streamed medium pass with
    its deferred hash pass, and k_bound_chunks for every medium chunk
    (DPG_MEDIUM_STREAM=0).  The PER_PRIVACY_ID modes run the hash kernels
    only: wide chunks in k_bound_waves<true>, medium chunks in k_bound_chunks;
    no marker says that k_bound_chunks had chunks there (the stage exists in
    every run) -- the 700-record ids exceed a wave chunk's capacity in any
    mode, as the cross modes' markers show on this same input."""
    if mw == "single":
        monkeypatch.setenv("DPG_MW_OFF", "1")
    elif mw == "multiwave":
        monkeypatch.setenv("DPG_MW_MEDIUM", "1")
    elif mw == "hash_medium":
        monkeypatch.setenv("DPG_MEDIUM_STREAM", "0")
    st = _run(mode, "wide_medium")
    if ev.is_per_pid(mode):
        assert "bound.kernel=hash" in st
        assert "bound.multiwave" not in st and "bound.medium_deferred" not in st
        assert st["bound.medium"] > 0.0
        return
    assert ("bound.multiwave" in st) == (mw != "single")
    assert ("bound.medium_deferred" in st) == (mw in ("default", "single"))
    assert st["bound.wide"] > 0.0 and st["bound.medium"] > 0.0


@pytest.mark.parametrize("size", [600, 1000])
@pytest.mark.parametrize("mode", ev.CROSS_MODES)
def test_streamed_medium_chunks(built, mode, size):
    """k_bound_sorted tier 3 streaming one `size`-record id per fine bucket
    in pieces, and k_bound_chunks_deferred for the ids on three partitions (a
    restart, then a deferral): test_gpu_streamed_medium_chunks_match_oracle's
    input.  A pair streamed in pieces, restarted or deferred must still be
    clamped once."""
    st = _run(mode, f"streamed{size}")
    assert "bound.medium_deferred" in st


@pytest.mark.parametrize("over", ["stream", "heavy_filter"])
@pytest.mark.parametrize("mode", ev.CROSS_MODES)
def test_oversize_buckets(built, monkeypatch, mode, over):
    """Oversize buckets at a 64-record capacity
    (test_gpu_oversize_buckets_match_oracle's input): streamed by tier 3 with
    the three-partition ids handed back to k_bound_big, or cut by the heavy
    filter into heavy chunks (DPG_STREAM_OVER=0)."""
    monkeypatch.setenv("DPG_STREAM_OVER", "1" if over == "stream" else "0")
    st = _run(mode, "oversize", tuning=(1024, 64))
    assert ("heavy" in st) == (over == "heavy_filter")
    assert "bound.medium" in st


@pytest.mark.parametrize("mode", _modes("global"))
def test_global_path(built, monkeypatch, mode):
    """k_bound_big for every record (test_gpu_global_path_item_types' input
    and hooks: a 64-record bucket capacity under ~100-record ids, the heavy
    filter off), with its three per-partition clipping sites.  No stage
    marker names k_bound_big; the absent heavy stage shows the filter was
    off, which leaves that kernel as the oversize buckets' only path."""
    monkeypatch.setenv("DPG_NO_HEAVY", "1")
    st = _run(mode, "global", tuning=(1024, 64))
    assert "heavy" not in st


@pytest.mark.parametrize("target,cap", [(16, 2048), (8, 48)], ids=["3levels", "mixed"])
@pytest.mark.parametrize("mode", _modes("levels"))
def test_partition_levels_and_refine(built, mode, target, cap):
    """Three partition levels, and the refine level mixed with the oversize
    paths (test_gpu_partition_levels_and_fallback's input and tunings).  No
    stage marker tells the level count apart; the tunings are the source
    test's."""
    _run(mode, "levels", tuning=(target, cap))


@pytest.mark.parametrize("mode", _modes("wide_records"))
def test_wide_records(built, mode):
    """12-byte records and the 256-thread chunk kernel for every bucket
    (test_gpu_wide_records' input: ids over 2^31 values, 4e7 partitions).  No
    stage marker names the record layout; it follows from the key widths."""
    _run(mode, "wide_records")


@pytest.mark.parametrize("gen", ["merge_uniform", "merge_hot"])
@pytest.mark.parametrize("mode", _modes("merge_uniform"))
def test_two_level_merge(built, mode, gen):
    """k_reduce_items behind two item levels (P = 6e6: 1465 ranges) for the
    24- and 32-byte items and for clamped pair sums: ranges of one tile,
    written by plain stores (uniform keys), and a range of several tiles,
    merged by global atomics (every key below 4096).  The items2 stage shows
    the second level; which store branch a range takes has no marker and
    follows from its kept pairs (test_merge_inputs_reach_both_branches)."""
    st = _run(mode, gen)
    assert "items2:hist" in st
