"""The public pre-aggregation (API mirror of analysis/pre_aggregation.py:19-61).

preaggregate() returns one row per (privacy id, partition) pair present in the
data, (partition_key, (count, sum, n_partitions, n_contributions)), for the
partitions the sampler keeps; n_partitions and n_contributions are the privacy
id's totals over ALL its partitions, sampled or not
(analysis/contribution_bounders.py:60-70).  The rows are what
perform_utility_analysis(pre_aggregated_data=True) and
compute_dataset_histograms_on_preaggregated_data take.

On the device that is pre_aggregation.device_pairs (dpg_preaggregate: every
pair, sorted by partition), the sampler's bitmap (dpg_sample_partitions for
integer keys) and a compaction of the pairs by their partition's bit.  The
pre-aggregation itself is not thinned: a privacy id's totals need all its
pairs.
"""
from typing import Any, Dict, Iterator, Tuple

import numpy as np
import torch

from pipelinedp_amd import columnar
from pipelinedp_amd import pipeline_backend
from pipelinedp_amd import pre_aggregation as device_pre
from pipelinedp_amd.analysis import utility_analysis


class PreAggregate:
    """Lazy result of preaggregate(): iterate it for the reference's rows, or
    take columns() for device tensors (1e8 pairs are not Python rows)."""

    def __init__(self, col, backend, data_extractors, partitions_sampling_prob):
        self._args = (col, backend, data_extractors)
        self._prob = partitions_sampling_prob
        self._cols = None

    def columns(self) -> Dict[str, Any]:
        """{"pk": dense partition ids (device int64), "count" (int64), "sum"
        (float64), "n_partitions", "n_contributions" (int64), "key_table":
        dense id -> key as columnar.decode_keys takes it (None: identity)},
        one entry per kept pair, sorted by pk."""
        if self._cols is None:
            self._cols = self._run()
        return self._cols

    def _run(self) -> Dict[str, Any]:
        col, backend, extractors = self._args
        dev = backend.device
        ps = device_pre.device_pairs(col, extractors, backend, None, dev)
        n, P = ps.n_pairs, ps.n_partitions
        words = ps.pairs[:n].view(torch.int32)           # [n, 6] words of dpg_pair_entry
        u32 = lambda w: words[:, w].to(torch.int64) & 0xFFFFFFFF
        pk = u32(0)
        keep = None
        if self._prob < 1:
            bound = utility_analysis._sample_bound(self._prob)
            if device_pre.integer_keys(ps.key_table):
                mask = device_pre.device_sample_mask(backend, dev, P, ps.key_table, None, bound)
            else:  # other key types: the host hash of each key's repr
                keys = columnar.decode_keys(np.arange(P), ps.key_table)
                bits = np.array([utility_analysis._keep_by_hash(k, bound) for k in keys], bool)
                mask = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
            keep = ((mask[pk >> 3].to(torch.int64) >> (pk & 7)) & 1).bool()
        sel = (lambda t: t[keep]) if keep is not None else (lambda t: t.clone())
        return dict(pk=sel(pk), count=sel(u32(1)), sum=sel(ps.pairs[:n, 1]),
                    n_partitions=sel(u32(4)), n_contributions=sel(u32(5) & device_pre.NC_MASK),
                    key_table=ps.key_table)

    def __iter__(self) -> Iterator[Tuple[Any, Tuple[int, float, int, int]]]:
        c = self.columns()
        keys = columnar.decode_keys(c["pk"].cpu().numpy(), c["key_table"])
        cols = [c[f].cpu().tolist() for f in ("count", "sum", "n_partitions", "n_contributions")]
        return zip(keys, zip(*cols))


def preaggregate(col, backend, data_extractors, partitions_sampling_prob: float = 1):
    """(partition_key, (count, sum, n_partitions, n_contributions)) per
    (privacy id, partition) pair of `col`, lazily; with
    partitions_sampling_prob < 1 only the partitions the deterministic sampler
    keeps (the same ones perform_utility_analysis keeps)."""
    if not isinstance(backend, pipeline_backend.MI355XBackend):
        raise NotImplementedError("analysis.preaggregate runs on MI355XBackend only")
    pipeline_backend.require_one_process(backend, "analysis.preaggregate")
    if not 0 < partitions_sampling_prob <= 1:
        raise ValueError(f"partitions_sampling_prob must be in the interval (0, 1], "
                         f"but {partitions_sampling_prob} given.")
    return PreAggregate(col, backend, data_extractors, partitions_sampling_prob)
