"""The team level 2 on the pieces of the histogram-free level 1: a member's
share of a bucket is resolved to its pieces once (dpg_team.h team_resolve).
A share inside one piece or across one piece boundary -- every share of a
bucket whose eight pieces are near-equal -- is loaded by the pair arm (one
compare per load); a share that spans more pieces takes the 8-piece lookup.
DPG_DEBUG_TEAM_PATHS=1 makes the call name the arms its members took as
zero-length stages "team.pieces=pair" / "team.pieces=lookup".

Level 1 scatters tile t (8192 records) by a workgroup of XCD t mod 8, so the
pieces of a bucket are its records in the tiles of each residue mod 8: the
cases below place privacy ids by tile residue to shape the pieces.  With
DPG_DEBUG_TARGET=1 and a declared range of 2^22 privacy ids the plan takes
11 + 11 bits, so a level-1 bucket holds a few privacy ids only.

Every case compares the partials with the oracle (privacy-id counts and
counts bit-exact, sums to 1e-9) and asserts the stages its path names.  The
resolution itself is compared with the 8-piece chain, index by index, on the
host (no GPU) through the library's debug export."""
import ctypes

import numpy as np
import pytest

SEED = 0x7EA3
SUB = 8 * 1024
N0 = 1 << 22
P = 100_000
U = 50_000
WIDE = 1 << 22  # declared privacy-id range of the sparse-bucket cases
T = 32          # members per team on 256 CUs


def _params(pdp, mpc=8, mcpp=2):
    return pdp.AggregateParams(
        metrics=[pdp.Metrics.COUNT, pdp.Metrics.SUM, pdp.Metrics.PRIVACY_ID_COUNT],
        noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=mpc,
        max_contributions_per_partition=mcpp, min_value=0.0, max_value=10.0)


def _run_and_check(pid, pk, val, pid_range):
    import torch
    import pipelinedp_amd as pdp
    from oracle import oracle
    backend = pdp.MI355XBackend(device=0, seed=SEED)
    acc = pdp.NaiveBudgetAccountant(1.0, 1e-6)
    cols = pdp.ColumnarData(pid=torch.from_numpy(pid).cuda(), pk=torch.from_numpy(pk).cuda(),
                            value=torch.from_numpy(val).cuda(), n_partitions=P,
                            privacy_id_range=pid_range)
    res = pdp.DPEngine(acc, backend).aggregate(cols, _params(pdp), pdp.DataExtractors("pid", "pk", "value"))
    acc.compute_budgets()
    res.noise_enabled = False
    res.nonce = 77
    res.materialize()
    got = {k: v.cpu().numpy() for k, v in res.last_partials.items() if v is not None}
    ref = oracle.bound_aggregate(pid, pk, val, res.last_bound_fields, SEED)
    assert np.array_equal(got["rows"], ref["rows"])
    assert np.array_equal(got["count"], ref["count"])
    assert np.allclose(got["sum"], ref["sum"], rtol=1e-9, atol=1e-9)
    return backend.ctx.stage_times()


def _assert_team_on_pieces(st):
    assert "partition1:pieces" in st and "partition2:team" in st
    assert "partition1:hist" not in st and "partition2:hist" not in st


@pytest.fixture(scope="module")
def balanced():
    """The bench generator: every bucket's pieces are near-equal."""
    import bench
    pid, pk, val = bench.host_sample(N0 + SUB + 2, U, P, 909)
    return pid.astype(np.int64), pk.astype(np.int64), val


def _keys_values(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, P, n).astype(np.int64), rng.uniform(-1.0, 11.0, n)


def _slots_by_residue(n, rng):
    """Record positions by the XCD (tile index mod 8) that scatters them."""
    res = (np.arange(n) // SUB) % 8
    return [rng.permutation(np.flatnonzero(res == r)) for r in range(8)]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [1, SUB + 2], ids=["odd", "even"])
def test_balanced_pieces_take_the_pair_arm(built, balanced, monkeypatch, extra):
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    monkeypatch.setenv("DPG_DEBUG_TEAM_PATHS", "1")
    pid, pk, val = (a[:N0 + extra] for a in balanced)
    st = _run_and_check(pid, pk, val, (0, U))
    _assert_team_on_pieces(st)
    assert "team.pieces=pair" in st


@pytest.mark.gpu
def test_share_over_more_than_two_pieces_takes_the_lookup(built, monkeypatch):
    """5000 privacy ids of 700 records each, id j's records all in the tiles
    of one XCD (residue j mod 8), over a thin uniform background (~340
    records, ~42 per piece, per bucket): a bucket is two or three large
    pieces and small ones in between, and a share (~64 records) that starts
    in the small ones covers a whole piece and parts of its neighbours.
    (A few dozen such ids over a uniform background of 2^22 records do not
    reach the lookup: every piece then holds more records than a share, so
    the one-XCD ids are the bulk of the input here.  At most 4416 records fit one region: seven ids of one residue would
    have to meet in one of the 2048 buckets to overflow it.)"""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    monkeypatch.setenv("DPG_DEBUG_TEAM_PATHS", "1")
    monkeypatch.setenv("DPG_DEBUG_TARGET", "1")
    n, k_ids, h = N0 + 3, 5000, 700
    rng = np.random.default_rng(4242)
    pid = rng.integers(WIDE // 2, WIDE, n)  # the background
    heavy = rng.choice(WIDE // 2, k_ids, replace=False)
    for r, slots in enumerate(_slots_by_residue(n, rng)):
        ids = heavy[r::8]
        assert len(ids) * h <= len(slots)
        pid[slots[:len(ids) * h]] = np.repeat(ids, h)
    pk, val = _keys_values(n, 4243)
    st = _run_and_check(pid.astype(np.int64), pk, val, (0, WIDE))
    _assert_team_on_pieces(st)
    assert "team.pieces=lookup" in st


@pytest.mark.gpu
def test_buckets_smaller_than_the_team(built, monkeypatch):
    """1500 privacy ids of ~2800 records and 300 of 1 to 40 records in 2048
    buckets: about half the buckets are empty, and a bucket that holds only
    a small id gives most of the 32 members no record (lim == 0) and the
    others one pair."""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    monkeypatch.setenv("DPG_DEBUG_TEAM_PATHS", "1")
    monkeypatch.setenv("DPG_DEBUG_TARGET", "1")
    n = N0 + 2
    rng = np.random.default_rng(5151)
    ids = rng.choice(WIDE, 1800, replace=False)
    pid = ids[rng.integers(0, 1500, n)]
    pos = rng.permutation(n)
    at = 0
    for j in range(300):
        c = 1 + j % 40
        pid[pos[at:at + c]] = ids[1500 + j]
        at += c
    pk, val = _keys_values(n, 5152)
    st = _run_and_check(pid.astype(np.int64), pk, val, (0, WIDE))
    _assert_team_on_pieces(st)
    assert "team.pieces=pair" in st


@pytest.mark.gpu
def test_buckets_with_empty_pieces(built, monkeypatch):
    """2800 privacy ids, each with records in the tiles of three XCDs only:
    a bucket of one id has five empty pieces, and its shares cross from one
    piece to the next non-empty one over the empty ones between."""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    monkeypatch.setenv("DPG_DEBUG_TEAM_PATHS", "1")
    monkeypatch.setenv("DPG_DEBUG_TARGET", "1")
    n, k_ids = N0 + 1, 2800
    rng = np.random.default_rng(6161)
    ids = rng.choice(WIDE, k_ids, replace=False)
    home = np.stack([rng.permutation(8)[:3] for _ in range(k_ids)])  # [k_ids, 3] residues
    pid = np.empty(n, dtype=np.int64)
    for r, slots in enumerate(_slots_by_residue(n, rng)):
        here = ids[(home == r).any(axis=1)]
        pid[slots] = here[np.arange(len(slots)) % len(here)]
    pk, val = _keys_values(n, 6162)
    st = _run_and_check(pid, pk, val, (0, WIDE))
    _assert_team_on_pieces(st)
    assert "team.pieces=pair" in st


@pytest.mark.gpu
def test_multi_round_launch_scans(built, balanced, monkeypatch):
    """DPG_DEBUG_TEAM_SUB=64: every bucket (~1000 records per member) goes
    through the multi-round launch, whose block scans use the same helper."""
    monkeypatch.setenv("DPG_L1_PIECES", "1")
    monkeypatch.setenv("DPG_DEBUG_TEAM_SUB", "64")
    pid, pk, val = (a[:N0 + 1] for a in balanced)
    st = _run_and_check(pid, pk, val, (0, U))
    _assert_team_on_pieces(st)
    assert "partition2:team_multi" in st


# ---------------------------------------------------------------- host: team_resolve

def _chain(ppre, i):
    """The 8-piece chain: the last piece p with i >= ppre[p]."""
    p = 0
    for q in range(1, 8):
        if i >= ppre[q]:
            p = q
    return p


def _descriptor(rng, counts):
    """ppre / dl / cend of pieces with the given record counts (each piece
    padded to an even length; dl arbitrary 32-bit offsets)."""
    ppre, ce, acc = [], [], 0
    for c in counts:
        ppre.append(acc)
        ce.append(acc + c)
        acc += (c + 1) & ~1
    dl = [int(x) for x in rng.integers(0, 1 << 32, 8)]
    return ppre, dl, ce, acc


def test_resolution_equals_the_chain_on_the_host(built):
    from pipelinedp_amd import _native
    lib = ctypes.CDLL(_native.library_path())
    u32, arr8, arr6 = ctypes.c_uint32, ctypes.c_uint32 * 8, ctypes.c_uint32 * 6
    lib.dpg_debug_team_resolve.argtypes = [arr8, arr8, arr8, u32, u32, arr6]
    lib.dpg_debug_team_resolve.restype = None
    rng = np.random.default_rng(7171)
    cases = [[5, 0, 0, 3, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 9], [1] * 8, [2] * 8, [0] * 7 + [1],
             [130, 2, 2, 2, 2, 2, 2, 2], [700, 41, 0, 43, 700, 0, 37, 45], [4001] * 8]
    for _ in range(60):
        size = int(rng.choice([3, 40, 600, 5000]))
        c = rng.integers(0, size, 8)
        c[rng.random(8) < 0.3] = 0  # empty pieces
        if c.sum() == 0:
            c[int(rng.integers(0, 8))] = 1
        cases.append([int(x) for x in c])
    n_pair = n_lookup = 0
    for counts in cases:
        ppre, dl, ce, n = _descriptor(rng, counts)
        q = ((n + T - 1) // T + 1) & ~1
        shares = [(min(n, m * q), min(n, min(n, m * q) + q) - min(n, m * q)) for m in range(T)]
        shares += [(0, n), (n - 2, 2), (n, 0)]  # the whole bucket, its end, past its end
        for b0, lim in shares:
            out = arr6()
            lib.dpg_debug_team_resolve(arr8(*ppre), arr8(*dl), arr8(*ce), b0, lim, out)
            bnd, dl0, ce0, dl1, ce1, pair = list(out)
            idx = range(b0, b0 + max(lim, 2) - 1, 2)
            pieces = [_chain(ppre, i) for i in idx]
            assert (dl0, ce0) == (dl[pieces[0]], ce[pieces[0]])
            assert (dl1, ce1) == (dl[pieces[-1]], ce[pieces[-1]])
            assert bnd == ppre[pieces[-1]]
            assert pair == (1 if len(set(pieces)) <= 2 else 0), (counts, b0, lim)
            if pair:
                n_pair += 1
                for i, p in zip(idx, pieces):
                    assert ((dl1, ce1) if i >= bnd else (dl0, ce0)) == (dl[p], ce[p]), (counts, b0, lim, i)
            else:
                n_lookup += 1
    assert n_pair > 100 and n_lookup > 20
