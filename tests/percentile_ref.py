"""Checkers of the percentile tests (not collected): the kept records of
contribution bounding restated from the oracle's priorities, and the
quantile-tree walk restated in numpy.  PyDP is not importable here, so this
restatement of the issue's text -- not PyDP -- is what the GPU is pinned to."""
import math

import numpy as np

from oracle import oracle

H, B, L = 4, 16, 65536
ALPHA, TOL = 0.0075, 1e-6
SLOT_QNODE0 = 16
MODE_CROSS_AND_PER, MODE_CROSS = 0, 2


def kept_records(pid, pk, fields, seed, public=None):
    """uint8[n]: the records dpg_bound_aggregate keeps (oracle/dp_oracle.c
    dpo_bound_aggregate_ids): pairs of a privacy id ascending by
    (pair_prio << 32 | pk), the first mpc; records of a pair ascending by
    rec_prio, the first mcpp (all of them in cross-partition mode)."""
    ss = oracle.stream_seed(seed, fields.get("nonce", 0))
    off = fields.get("rec_id_offset", 0)
    mpc = fields["max_partitions_contributed"]
    mcpp = fields["max_contributions_per_partition"]
    public = None if public is None else set(int(k) for k in public)
    pairs = {}
    for i, (p, k) in enumerate(zip(pid.tolist(), pk.tolist())):
        if public is not None and k not in public:
            continue
        pairs.setdefault(p, {}).setdefault(k, []).append(i)
    keep = np.zeros(len(pid), np.uint8)
    for p, by_pk in pairs.items():
        order = sorted(by_pk, key=lambda k: (oracle.pair_prio(ss, p, k) << 32) | k)
        for k in order[:mpc]:
            recs = by_pk[k]
            if fields["mode"] != MODE_CROSS:
                recs = sorted(recs, key=lambda i: oracle.rec_prio(ss, p, k, off + i))[:mcpp]
            keep[recs] = 1
    return keep


def leaf_of(v, lo, hi):
    v = np.asarray(v, dtype=np.float64)
    if not hi > lo:
        return np.zeros(len(v), np.int64)
    x = np.floor((np.clip(v, lo, hi) - lo) * float(L) / (hi - lo))
    return np.minimum(L - 1, x).astype(np.int64)


def quantiles(values, qs, lo, hi, noised=None, stats=None):
    """The walk of one partition over its kept values (NaN ignored).
    noised(node, count) -> noised count (None: noise-free).  Returns the
    quantiles and the smallest |partial / T' - (rank - tau)| a branch
    decision met (inf if none was taken).  stats (a dict) counts the node
    counts clamped at 0 and the positive ones the alpha filter dropped."""
    values = np.asarray(values, dtype=np.float64)
    values = values[~np.isnan(values)]
    cum = np.concatenate([[0], np.cumsum(np.bincount(leaf_of(values, lo, hi), minlength=L))])
    w = (hi - lo) / float(L)
    cache = {}

    def count(nu, c):
        if noised is None:
            return c
        if nu not in cache:
            cache[nu] = noised(nu, c)
        return cache[nu]

    out, margin = [], math.inf
    for q in qs:
        rank, level, node = float(q), 0, 0
        for lvl in range(1, H + 1):
            span = B ** (H - lvl)
            first = (B ** lvl - 1) // (B - 1)
            raw = np.array([count(first + node * B + i,
                                  float(cum[(node * B + i + 1) * span] - cum[(node * B + i) * span]))
                            for i in range(B)])
            c = np.maximum(0.0, raw)
            T = c.sum()
            cf = np.where(c >= ALPHA * T, c, 0.0)
            if stats is not None:
                stats["clamped"] = stats.get("clamped", 0) + int((raw < 0).sum())
                stats["filtered"] = stats.get("filtered", 0) + int(((c > 0) & (cf == 0)).sum())
            S = np.cumsum(cf)
            Tf = S[-1]
            if not Tf > 0.0:
                break
            pick = B - 1
            for i in range(B):
                margin = min(margin, abs(S[i] / Tf - (rank - TOL)))
                if S[i] / Tf >= rank - TOL:
                    pick = i
                    break
            ci = cf[pick]
            r = (rank - (S[pick] - ci) / Tf) / (ci / Tf) if ci > 0.0 else 0.0
            rank = min(1.0, max(0.0, r))
            level, node = lvl, node * B + pick
        span = B ** (H - level)
        left, right = lo + float(node * span) * w, lo + float((node + 1) * span) * w
        out.append((1.0 - rank) * left + rank * right)
    return np.array(out), margin


def oracle_noise(kind, scale, stream_seed, k_global):
    """noised(node, count) of partition k_global from the oracle's sampler."""
    return lambda nu, c: oracle.noise_sample(kind, c, scale, stream_seed, k_global,
                                             SLOT_QNODE0 + nu)


def order_statistic(values, q, lo, hi):
    """The clamped value the walk's result shares a leaf with: element
    ceil(q n - tau n) (1-based, at least 1) of the sorted kept values."""
    x = np.sort(np.clip(values[~np.isnan(values)], lo, hi))
    m = max(1, math.ceil(q * len(x) - TOL * len(x)))
    return x[m - 1]
