"""The bounding sort on 32-bit keys (dpg_sortb.h, phase S): pid slot |
truncated pair priority | candidate position, one v_med3_u32 per cross-lane
compare-exchange.  A chunk whose truncated priorities tie two pairs of one
privacy id the wrong way round fails the ascending-full-key check and is
sorted again by the float64-packed network, so in every case below the
partials must equal the oracle's bit for bit (sums to 1e-9): with the
priority bits capped at 2 (DPG_DEBUG_SORT32_PPB) nearly every chunk takes
that fallback, so parity there is the evidence that check and fallback work.
Every case runs with noise off and two release nonces (two samplings)."""
import numpy as np
import pytest
import torch

import bench
import pipelinedp_amd as pdp
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = 0x50B732
NONCES = (0x32A, 0x32B)


def _csp(mpc, mcpp):
    return dict(metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
                max_partitions_contributed=mpc, max_contributions_per_partition=mcpp,
                min_value=0.0, max_value=10.0)


def _check(pid, pk, val, P, kw):
    """One aggregate per nonce: partials against the oracle, and the marker
    of a launch with the 32-bit path compiled in."""
    pid, pk = pid.astype(np.int64), pk.astype(np.int64)
    mask = oracle.bitmap(range(P), P)
    for nonce in NONCES:
        backend = pdp.MI355XBackend(device=0, seed=SEED)
        acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
        res = pdp.DPEngine(acc, backend).aggregate(
            pdp.ColumnarData(pid=torch.as_tensor(pid), pk=torch.as_tensor(pk),
                             value=torch.as_tensor(val), n_partitions=P),
            pdp.AggregateParams(**kw), pdp.DataExtractors("pid", "pk", "value"),
            public_partitions=list(range(P)))
        acc.compute_budgets()
        res.noise_enabled = False
        res.nonce = nonce
        res.materialize()
        st = backend.ctx.stage_times()
        assert "bound.kernel=sort" in st
        assert "bound.sort32" in st
        ref = oracle.bound_aggregate(pid, pk, val if res.plan.needs_values() else None,
                                     res.last_bound_fields, SEED, public_mask=mask)
        got = {k: (v.cpu().numpy() if v is not None else None)
               for k, v in res.last_partials.items()}
        assert np.array_equal(got["rows"], ref["rows"])
        assert np.array_equal(got["count"], ref["count"])
        for k in ("sum", "nsum", "nsq"):
            if got[k] is not None:
                assert np.allclose(got[k], ref[k], rtol=1e-9, atol=1e-9), k
    return st


@pytest.fixture(scope="module")
def flagship_small():
    return bench.host_sample(1_000_000, 10_000, 100_000, 3232)


@pytest.mark.parametrize("cap", [None, "2"], ids=["default", "ppb2_fallback"])
def test_sort32_flagship_shape(built, monkeypatch, flagship_small, cap):
    """The bench's generator and bounds (mpc 8, mcpp 2) at 1e6 records: the
    default path, and the same with 2 priority bits kept (fallback)."""
    monkeypatch.delenv("DPG_DEBUG_SORT32_PPB", raising=False)
    if cap:
        monkeypatch.setenv("DPG_DEBUG_SORT32_PPB", cap)
    pid, pk, val = flagship_small
    _check(pid, pk, val, 100_000, _csp(8, 2))


def test_sort32_many_candidates_per_id(built, monkeypatch):
    """20 000 privacy ids of 200 records on 200 distinct partitions each, mpc
    64, mcpp 1: two filtered ids of ~111 candidates fill a 256-element sort
    that keeps 23 priority bits, so ~111^2 / 2^24 = 7e-4 of the ids tie two
    pairs by chance -- natural fallbacks."""
    monkeypatch.delenv("DPG_DEBUG_SORT32_PPB", raising=False)
    rng = np.random.default_rng(64)
    n_pid, per, P = 20_000, 200, 100_000
    pid = np.repeat(np.arange(n_pid), per)
    # distinct per id: an arithmetic progression that does not wrap round P
    base, step = rng.integers(0, P, (n_pid, 1)), rng.integers(1, P // per, (n_pid, 1))
    pk = ((base + step * np.arange(per)) % P).ravel()
    perm = rng.permutation(pid.size)
    pid, pk = pid[perm], pk[perm]
    val = rng.uniform(-2.0, 12.0, pid.size)
    _check(pid, pk, val, P, _csp(64, 1))


def test_sort32_tiny_ids(built, monkeypatch):
    """200 000 records over 100 000 privacy ids, mpc 8: chunks of many tiny
    ids occupy all 128 pid slots (7 slot bits), which leaves a 256-element
    sort 17 priority bits, the fewest any chunk keeps -- at the threshold
    kSort32MinPpb (a threshold of 18 sends these chunks to the float64
    network first; measured slower)."""
    monkeypatch.delenv("DPG_DEBUG_SORT32_PPB", raising=False)
    rng = np.random.default_rng(7)
    n, P = 200_000, 50_000
    pid = rng.integers(0, 100_000, n)
    pk = (rng.zipf(1.2, n) - 1) % P
    val = rng.uniform(-2.0, 12.0, n)
    _check(pid, pk, val, P, _csp(8, 2))


@pytest.mark.parametrize("cap", [None, "2"], ids=["default", "ppb2_fallback"])
def test_sort32_streamed_pass(built, monkeypatch, cap):
    """1 000 privacy ids of ~700 records each, mpc 8, mcpp 2: medium chunks,
    streamed by tier 3 through the same sort_chunk."""
    for v in ("DPG_DEBUG_SORT32_PPB", "DPG_MW_MEDIUM", "DPG_MEDIUM_STREAM"):
        monkeypatch.delenv(v, raising=False)
    if cap:
        monkeypatch.setenv("DPG_DEBUG_SORT32_PPB", cap)
    rng = np.random.default_rng(700)
    P = 20_000
    pid = np.repeat(np.arange(1000), rng.integers(650, 750, 1000))
    pk = (rng.zipf(1.1, pid.size) - 1) % P
    perm = rng.permutation(pid.size)
    pid, pk = pid[perm], pk[perm]
    val = rng.uniform(-2.0, 12.0, pid.size)
    st = _check(pid, pk, val, P, _csp(8, 2))
    assert st["bound.medium"] > 0.0


def test_sort32_mean_variance(built, monkeypatch, flagship_small):
    """The flagship shape with MEAN + VARIANCE (Gaussian): the same
    sort_chunk with the 24-byte ItemV items."""
    monkeypatch.delenv("DPG_DEBUG_SORT32_PPB", raising=False)
    pid, pk, val = flagship_small
    kw = dict(metrics=[pdp.Metrics.MEAN, pdp.Metrics.VARIANCE],
              noise_kind=pdp.NoiseKind.GAUSSIAN, max_partitions_contributed=8,
              max_contributions_per_partition=2, min_value=0.0, max_value=10.0)
    _check(pid, pk, val, 100_000, kw)
