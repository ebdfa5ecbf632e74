"""The key set of the partition-sampler tests (test_gpu_partition_sampler.py,
test_sampler_host.py): every decimal digit-count boundary of int64, the
32- and 53-bit edges, the extremes, and seeded random keys."""
import random


def edge_keys():
    ks = [0, 1, -1, 9, -9, 10, -10]
    for k in range(1, 19):
        ks += [10**k - 1, -(10**k - 1), 10**k, -(10**k)]
    ks += [2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**53 + 1, 2**63 - 1, -2**63]
    return ks


def random_keys(n=4096, seed=20):
    r = random.Random(seed)
    return [r.randrange(-2**63, 2**63) for _ in range(n)]
