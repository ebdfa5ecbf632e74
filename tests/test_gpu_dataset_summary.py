"""analysis.dataset_summary on the GPU (dpg_partition_summary): the
reference's own known answer, columnar input with the public partitions in
every form the ingest takes, and an out-of-range key."""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import analysis
from pipelinedp_amd.analysis import dataset_summary

pytestmark = pytest.mark.gpu


def _backend():
    return pdp.MI355XBackend(device=0, seed=7)


def test_exports():
    assert analysis.dataset_summary is dataset_summary
    assert callable(analysis.preaggregate)


def test_reference_known_answer(built):
    """analysis/tests/dataset_summary_test.py: rows 0 .. 99, public 60 .. 120."""
    ex = pdp.DataExtractors(privacy_id_extractor=lambda x: x, partition_extractor=lambda x: x,
                            value_extractor=lambda x: 0)
    (s,) = list(dataset_summary.compute_public_partitions_summary(
        list(range(100)), _backend(), ex, list(range(60, 121))))
    assert s == dataset_summary.PublicPartitionsSummary(
        num_dataset_public_partitions=40, num_dataset_non_public_partitions=60,
        num_empty_public_partitions=21)


def test_string_keys(built):
    ex = pdp.DataExtractors(partition_extractor=lambda x: f"pk{x}")
    (s,) = list(dataset_summary.compute_public_partitions_summary(
        [0, 1, 1, 2, 5], _backend(), ex, ["pk1", "pk5", "pk7"]))
    assert (s.num_dataset_public_partitions, s.num_dataset_non_public_partitions,
            s.num_empty_public_partitions) == (2, 2, 1)


N, P = 200_000, 100_003


@pytest.fixture(scope="module")
def columns():
    rng = np.random.default_rng(33)
    pk = rng.integers(0, P, N)
    pk[:5] = [0, 7, 8, P - 2, P - 1]      # the bitmap's first bytes and last, partial byte
    return pk, np.unique(pk)


@pytest.mark.parametrize("form", ["range", "tensor", "list"])
def test_columnar_matches_set_arithmetic(built, columns, form):
    pk, present = columns
    if form == "range":
        public = range(1_000, 90_001)
        pub = np.arange(1_000, 90_001)
    else:
        pub = np.unique(np.random.default_rng(34).integers(0, P, 60_000))
        pub = np.union1d(pub, [0, P - 1])
        public = torch.as_tensor(pub) if form == "tensor" else pub.tolist()
    cols = pdp.ColumnarData(pk=torch.as_tensor(pk), n_partitions=P)
    (s,) = list(dataset_summary.compute_public_partitions_summary(
        cols, _backend(), pdp.DataExtractors(partition_extractor="pk"), public))
    both = len(np.intersect1d(present, pub))
    assert (s.num_dataset_public_partitions, s.num_dataset_non_public_partitions,
            s.num_empty_public_partitions) == (both, len(present) - both, len(pub) - both)
    assert 0 < both < len(present) and both < len(pub)


def test_out_of_range_key_raises(built):
    pk = torch.as_tensor(np.array([0, 1, 2, 10, 3], np.int64))
    cols = pdp.ColumnarData(pk=pk, n_partitions=10)
    with pytest.raises(ValueError, match="outside"):
        list(dataset_summary.compute_public_partitions_summary(
            cols, _backend(), pdp.DataExtractors(partition_extractor="pk"), range(0, 5)))
    cols = pdp.ColumnarData(pk=torch.as_tensor(np.array([0, -1], np.int64)), n_partitions=10)
    with pytest.raises(ValueError, match="outside"):
        list(dataset_summary.compute_public_partitions_summary(
            cols, _backend(), pdp.DataExtractors(partition_extractor="pk"), range(0, 5)))
