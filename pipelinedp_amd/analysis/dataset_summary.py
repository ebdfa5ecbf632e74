"""How a public-partition list relates to the data (API mirror of
analysis/dataset_summary.py): how many of the dataset's partitions are
public, how many are not, and how many public partitions hold no data.

The reference groups the distinct dataset partitions and the public ones by
key.  Here the ingest (columnar.encode with the public list) gives dense ids
over the union and the public bitmap; dpg_partition_summary marks the ids the
data touches and counts the three classes in one pass over the partitions.
"""
import ctypes
import dataclasses

import torch

from pipelinedp_amd import columnar
from pipelinedp_amd import pipeline_backend
from pipelinedp_amd.analysis.utility_analysis import _Lazy


@dataclasses.dataclass
class PublicPartitionsSummary:
    num_dataset_public_partitions: int
    num_dataset_non_public_partitions: int
    num_empty_public_partitions: int


def compute_public_partitions_summary(col, backend, extractors, public_partitions):
    """A lazy 1-element collection holding the PublicPartitionsSummary of
    `col` (rows or columns, as DPEngine.aggregate takes them) against
    `public_partitions`.  With ColumnarData(n_partitions=P) every key, public
    ones included, must be a dense id in [0, P): ValueError otherwise."""
    if not isinstance(backend, pipeline_backend.MI355XBackend):
        raise NotImplementedError("compute_public_partitions_summary runs on MI355XBackend only")
    pipeline_backend.require_one_process(backend, "analysis.dataset_summary")
    if public_partitions is None:
        raise ValueError("public_partitions must be given")

    def run():
        dev = backend.device
        enc = columnar.encode(col, extractors, dev, need_values=False, need_pid=False,
                              public_partitions=public_partitions, ctx=backend.ctx)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            sptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            backend.ctx.partition_summary(
                ctypes.c_void_p(enc.pk.data_ptr()) if enc.n else None, enc.n, enc.n_partitions,
                ctypes.c_void_p(enc.public_mask.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
                sptr)
        return [PublicPartitionsSummary(*counts.tolist())]

    return _Lazy(run)
