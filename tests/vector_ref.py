"""Checkers of the VECTOR_SUM tests (not collected): the release's norm clip
restated in numpy and the oracle's keyed noise of one coordinate.  The kept
records are those of tests/percentile_ref.py."""
import numpy as np

from oracle import oracle
from tests.percentile_ref import kept_records  # noqa: F401  (shared with the vector tests)

SLOT_VEC0 = 1 << 20
VSUM_CHUNK = 512
NORM_LINF, NORM_L1, NORM_L2 = 0, 1, 2
NOISE_NONE, NOISE_LAPLACE, NOISE_GAUSSIAN = 0, 1, 2


def norm(s, kind):
    s = np.asarray(s, dtype=np.float64)
    if kind == NORM_L1:
        return float(np.abs(s).sum())
    if kind == NORM_L2:
        return float(np.sqrt((s * s).sum()))
    return float(np.abs(s).max()) if s.size else 0.0


def clip(s, max_norm, kind):
    """The summed vector of one partition as it is released before noise:
    linf clamps every coordinate; l1 / l2 scale by min(1, max_norm / norm),
    a zero vector stays as it is."""
    s = np.asarray(s, dtype=np.float64)
    if kind == NORM_LINF:
        return np.clip(s, -max_norm, max_norm)
    nrm = norm(s, kind)
    return s * (max_norm / nrm) if nrm > max_norm else s.copy()


def oracle_noise(kind, scale, stream_seed, k_global):
    """noised(d, x) of coordinate d of partition k_global from the oracle's sampler."""
    return lambda d, x: oracle.noise_sample(kind, float(x), scale, stream_seed, k_global,
                                            SLOT_VEC0 + d)


def partition_sums(pk, value, keep, P):
    """[P, D] sums of the kept rows, float64, in numpy's order."""
    out = np.zeros((P, value.shape[1]), np.float64)
    m = keep != 0
    np.add.at(out, pk[m], value[m])
    return out
