"""The histogram call in three phases through the C ABI (dpg_hist_pairs,
dpg_hist_partitions, dpg_hist_sums), one process:

* composed on one pre-aggregate they equal dpg_dataset_histograms on the same
  pairs: integer bins, LINF_SUM counts, edges and maxima bit for bit, the
  LINF_SUM sums (float atomics in either call) to 1e-9 relative;
* run per emulated rank (R = 2 and 3: the records split by shard_of, every
  shard pre-aggregated with the global P), with the per-partition totals added,
  the ranges reduced and the bins added / maxed with torch as the ranks'
  collectives would, they equal the oracle (oracle/hist_oracle.py) on the
  whole dataset -- exactly: the values are eighths, so every sum is exact in
  any order.

Edge cases: a rank without pairs, no pairs at all, five equal pair sums (zero
step), P = 5 on 3 ranks (unequal owned slices), and the top edge's bin."""
import ctypes

import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from oracle import hist_oracle
from pipelinedp_amd import _native
from pipelinedp_amd import pre_aggregation
from tests import hist_cases as hc

pytestmark = pytest.mark.gpu

EXC = pdp.DataExtractors(privacy_id_extractor="pid", partition_extractor="pk",
                         value_extractor="value")
NB, NS = _native.HIST_INT_BINS, _native.HIST_SUM_BINS
N_SMALL, P_SMALL = 20_000, 311


@pytest.fixture(scope="module")
def backend(built):
    return pdp.MI355XBackend(device=0, seed=3)


def small_dataset(exact=True):
    """The first records of the shared dataset (the wide privacy id's
    partitions folded into P_SMALL): L0 = 311 and LINF = 1200 included."""
    d = hc.dataset(exact)
    return d["pid"][:N_SMALL], d["pk"][:N_SMALL] % P_SMALL, d["value"][:N_SMALL]


def pairs_of(backend, pid, pk, val, P):
    """The pre-aggregate of these records under the global P (None: none)."""
    if len(pid) == 0:
        return None
    col = pdp.ColumnarData(pid=torch.from_numpy(np.array(pid)).cuda(),  # copies: writable
                           pk=torch.from_numpy(np.array(pk)).cuda(),
                           value=torch.from_numpy(np.array(val)).cuda(),
                           n_partitions=P)
    return pre_aggregation.device_pairs(col, EXC, backend, None, backend.device)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(ps):
    return (ps.pairs.data_ptr(), ps.n_pairs, ps.starts.data_ptr()) if ps else (None, 0, None)


def _outs():
    i64, f64 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.float64, device="cuda")
    # filled with ones: the calls zero-fill what they say they do
    return (torch.ones(NS, **i64), torch.ones(NS, **f64), torch.ones(NS, **f64),
            torch.ones(NS + 1, **f64))


def one_call(backend, ps, P):
    """dpg_dataset_histograms: (int_bins, sum_count, sum_sum, sum_max, lowers)."""
    ib = torch.ones((5, NB, 3), dtype=torch.int64, device="cuda")
    sc, ss, sm, lw = _outs()
    starts = ps.starts if ps else torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    out = _native.HistOut(ib.data_ptr(), sc.data_ptr(), ss.data_ptr(), sm.data_ptr(),
                          lw.data_ptr())
    backend.ctx.dataset_histograms(_ptr(ps)[0], _ptr(ps)[1], starts.data_ptr(), P, False, out,
                                   _stream())
    torch.cuda.synchronize()
    return ib, sc, ss, sm, lw


def phases(backend, shards, P):
    """The three phases over emulated ranks (shards: one PairSet or None per
    rank) with torch in the place of the collectives."""
    ctx, R = backend.ctx, len(shards)
    ibs, rows, counts, ranges = [], [], [], []
    for ps in shards:
        ib = torch.ones((5, NB, 3), dtype=torch.int64, device="cuda")
        r = torch.full((P,), -1, dtype=torch.int64, device="cuda")
        c = torch.full((P,), -1, dtype=torch.int64, device="cuda")
        rng = torch.zeros(2, dtype=torch.float64, device="cuda")
        pairs, n, starts = _ptr(ps)
        ctx.hist_pairs(pairs, n, starts, P, ib.data_ptr(), r.data_ptr(), c.data_ptr(),
                       rng.data_ptr(), _stream())
        if n == 0:
            assert rng.tolist() == [float("inf"), float("-inf")]
            assert not r.any() and not c.any() and not ib.any()
        ibs.append(ib), rows.append(r), counts.append(c), ranges.append(rng)
    rows, counts = torch.stack(rows).sum(0), torch.stack(counts).sum(0)
    ranges = torch.stack(ranges)
    whole = torch.stack([ranges[:, 0].min(), ranges[:, 1].max()]).contiguous()
    for r in range(R):  # the owner of r, r + R, ... bins their merged totals
        own_r, own_c = rows[r::R].contiguous(), counts[r::R].contiguous()
        assert own_r.numel() == len(range(r, P, R))
        ctx.hist_partitions(own_r.data_ptr() if own_r.numel() else None,
                            own_c.data_ptr() if own_c.numel() else None, own_r.numel(),
                            ibs[r].data_ptr(), _stream())
    ibs = torch.stack(ibs)
    ib = torch.cat([ibs[..., 0:2].sum(0), ibs[..., 2:3].max(0).values], -1)
    scs, sss, sms, lws = [], [], [], []
    for ps in shards:
        sc, ss, sm, lw = _outs()
        pairs, n, _ = _ptr(ps)
        ctx.hist_sums(pairs, n, whole.data_ptr(), sc.data_ptr(), ss.data_ptr(), sm.data_ptr(),
                      lw.data_ptr(), _stream())
        scs.append(sc), sss.append(ss), lws.append(lw)
        sms.append(torch.where(sc > 0, sm, torch.full_like(sm, float("-inf"))))
    for lw in lws[1:]:  # every rank holds the same edges, pairs or none
        assert torch.equal(lw, lws[0])
    sc = torch.stack(scs).sum(0)
    sm = torch.where(sc > 0, torch.stack(sms).max(0).values, torch.zeros_like(sms[0]))
    torch.cuda.synchronize()
    return ib, sc, torch.stack(sss).sum(0), sm, lws[0], whole


def plain(arrays):
    ib, sc, ss, sm, lw = (a.cpu().numpy() for a in arrays[:5])
    return hc.plain_raw(ib.view(np.uint64), sc, ss, sm, lw)


def shards_of(backend, pid, pk, val, P, R):
    owner = hc.shard_np(pid, R)
    return [pairs_of(backend, pid[owner == r], pk[owner == r], val[owner == r], P)
            for r in range(R)]


def test_composed_phases_equal_the_one_call(backend):
    pid, pk, val = small_dataset(exact=False)
    ps = pairs_of(backend, pid, pk, val, P_SMALL)
    want = one_call(backend, ps, P_SMALL)
    got = phases(backend, [ps], P_SMALL)
    assert want[1].sum().item() == ps.n_pairs > 0
    for name, a, b in zip(("int_bins", "sum_count", "sum_sum", "sum_max", "lowers"), got, want):
        if name == "sum_sum":
            assert torch.allclose(a, b, rtol=1e-9, atol=0.0), name
        else:
            assert a.view(torch.int64).equal(b.view(torch.int64)), name  # the bits
    stages = backend.ctx.stage_times()
    assert "hist.sums" in stages  # the last call's stages


@pytest.mark.parametrize("R", [2, 3])
def test_emulated_ranks_equal_the_oracle(backend, R):
    pid, pk, val = small_dataset()
    want = hc.as_lists(hist_oracle.dataset_histograms(pid, pk, val))
    got = plain(phases(backend, shards_of(backend, pid, pk, val, P_SMALL, R), P_SMALL))
    assert got == want
    # the width-1 LDS bins and the global-atomic bins (>= 1000) were both hit
    assert want[2][1][-1][0] >= 1000 and want[4][1][-1][0] >= 1000


def test_one_rank_without_pairs(backend):
    pid, pk, val = small_dataset()
    ps = pairs_of(backend, pid, pk, val, P_SMALL)
    want = hc.as_lists(hist_oracle.dataset_histograms(pid, pk, val))
    assert plain(phases(backend, [ps, None], P_SMALL)) == want
    assert plain(phases(backend, [None, ps, None], P_SMALL)) == want


def test_no_pairs_at_all(backend):
    got = phases(backend, [None, None], 7)
    assert got[5].tolist() == [float("inf"), float("-inf")]
    for a, b in zip(got[:5], one_call(backend, None, 7)):
        assert not a.any() and not b.any()


def test_equal_sums_zero_step(backend):
    pid, pk = np.arange(5, dtype=np.int64) * 977, np.array([0, 2, 2, 3, 4], dtype=np.int64)
    val = np.full(5, 2.5)
    want = hc.as_lists(hist_oracle.dataset_histograms(pid, pk, val))
    for R in (1, 2, 3):
        got = phases(backend, shards_of(backend, pid, pk, val, 5, R), 5)
        assert got[5].tolist() == [2.5, 2.5]
        assert plain(got) == want, R
    ps = pairs_of(backend, pid, pk, val, 5)
    assert plain(one_call(backend, ps, 5)) == want


def test_five_partitions_three_ranks_and_the_top_edge(backend):
    """P = 5, R = 3: the owned slices hold 2, 2 and 1 partitions.  The largest
    pair sum equals the top edge and lands in the last bin, on whichever rank
    holds it."""
    rng = np.random.default_rng(5)
    pid = rng.integers(0, 40, 600).astype(np.int64)
    pk = rng.integers(0, 5, 600).astype(np.int64)
    val = rng.integers(-8, 49, 600) / 8.0
    want = hc.as_lists(hist_oracle.dataset_histograms(pid, pk, val))
    got = phases(backend, shards_of(backend, pid, pk, val, 5, 3), 5)
    assert plain(got) == want
    top = want[3][1][-1]
    assert top[1] == top[4] == got[5][1].item() and got[1][-1].item() >= 1


def test_invalid_arguments(backend):
    ctx = backend.ctx
    buf = torch.zeros(16, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.hist_pairs(None, 3, p, 4, p, p, p, p, _stream())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.hist_pairs(None, 0, None, 0, p, p, p, p, _stream())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.hist_partitions(p, p, -1, p, _stream())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.hist_partitions(p, p, 1 << 32, p, _stream())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.hist_sums(None, 0, None, p, p, p, p, _stream())
