"""StringColumn on the host: construction, round trips, the sort-order claim
the device dictionary rests on, the option combinations it excludes, and the
numpy hash against the restatement of dpg.h in tests/string_ref.py.  No GPU."""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import columnar, distributed, string_columns
from pipelinedp_amd.string_columns import StringColumn
from tests import string_ref

WORDS = ["", "a", "é", "z", "€", "￿", "\U00010000", "plain ascii", "naïve café",
         "exactly8", "ninebytes", "日本語のキー", "a" * 63, "b" * 64, "c" * 65, ""]


def test_exported():
    assert pdp.StringColumn is StringColumn


def test_construction_errors():
    data = np.zeros(4, dtype=np.uint8)
    with pytest.raises(TypeError, match="offsets"):
        StringColumn(np.array([0.0, 4.0]), data)
    with pytest.raises(TypeError, match="offsets"):
        StringColumn(np.zeros((2, 2), dtype=np.int64), data)
    with pytest.raises(TypeError, match="offsets"):
        StringColumn(torch.tensor([0.0, 4.0]), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(TypeError, match="data"):
        StringColumn(np.array([0, 4]), np.zeros(4, dtype=np.int8))
    with pytest.raises(TypeError, match="data"):
        StringColumn(torch.tensor([0, 4]), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="n \\+ 1"):
        StringColumn(np.zeros(0, dtype=np.int64), data)
    assert len(StringColumn(np.array([0]), np.zeros(0, dtype=np.uint8))) == 0


def test_round_trip():
    col = StringColumn.from_strings(WORDS)
    assert len(col) == len(WORDS)
    assert col.offsets.dtype == np.int64 and col.data.dtype == np.uint8
    assert col.to_strings() == WORDS
    assert int(col.offsets[-1]) == len("".join(WORDS).encode("utf-8")) == col.data.size
    assert StringColumn.from_strings([]).to_strings() == []
    latin = StringColumn.from_strings(["é", "z"], encoding="latin-1")
    assert latin.data.size == 2 and latin.to_strings() == ["é", "z"]


def test_round_trip_of_views_and_int32_offsets():
    """Tensors, int32 offsets and an offset view of a larger buffer."""
    col = StringColumn.from_strings(WORDS)
    big = np.full(col.data.size + 10, 0xFF, dtype=np.uint8)
    big[3:3 + col.data.size] = col.data
    view = StringColumn(torch.from_numpy(col.offsets.astype(np.int32)),
                        torch.from_numpy(big)[3:3 + col.data.size])
    assert view.to_strings() == WORDS
    off, data = view.host_columns()
    assert off.dtype == np.int64 and data.flags.c_contiguous
    # every other offset of an interleaved array: a strided view
    inter = np.zeros(2 * len(col.offsets), dtype=np.int64)
    inter[::2] = col.offsets
    assert StringColumn(inter[::2], col.data).to_strings() == WORDS
    with pytest.raises(ValueError, match="ascending"):
        StringColumn(np.array([0, 5, 3]), np.zeros(8, dtype=np.uint8)).to_strings()


def test_utf8_byte_order_is_code_point_order():
    words = ["é", "z", "€", "￿", "\U00010000"]
    by_bytes = [b.decode("utf-8") for b in sorted(w.encode("utf-8") for w in words)]
    assert sorted(words) == by_bytes == ["z", "é", "€", "￿", "\U00010000"]
    # UTF-16 code units would put the astral character before U+FFFF
    assert sorted(words, key=lambda w: w.encode("utf-16-be")) != by_bytes


def test_columnar_combination_errors():
    pk = StringColumn.from_strings(["a", "b", "a"])
    pid = StringColumn.from_strings(["u", "v", "u"])
    ints = np.arange(3)
    with pytest.raises(ValueError, match="n_partitions"):
        pdp.ColumnarData(pid=ints, pk=pk, n_partitions=2)
    with pytest.raises(ValueError, match="sparse_partition_keys"):
        pdp.ColumnarData(pid=ints, pk=pk, sparse_partition_keys=True)
    with pytest.raises(ValueError, match="privacy_id_range"):
        pdp.ColumnarData(pid=pid, pk=ints, privacy_id_range=(0, 10))
    # the flag a string pid implies is accepted
    data = pdp.ColumnarData(pid=pid, pk=pk, wide_privacy_ids=True)
    assert len(data) == 3 and bool(data)
    with pytest.raises(ValueError, match="has 2 elements but pk has 3"):
        columnar._check_length("pid", StringColumn.from_strings(["u", "v"]), len(data))


def test_encode_needs_the_library_context_and_one_process():
    """Both raised from host state, before any device work."""
    ex = pdp.DataExtractors("pid", "pk", "value")
    dev = torch.device("cpu")
    pk = StringColumn.from_strings(["a", "b", "a"])
    pid = StringColumn.from_strings(["u", "v", "u"])
    ints = np.arange(3)
    with pytest.raises(NotImplementedError, match="library context"):
        columnar.encode(pdp.ColumnarData(pid=ints, pk=pk), ex, dev, need_values=False)
    with pytest.raises(NotImplementedError, match="library context"):
        columnar.encode(pdp.ColumnarData(pid=pid, pk=ints), ex, dev, need_values=False)
    with pytest.raises(NotImplementedError, match="one process"):
        columnar.encode(pdp.ColumnarData(pid=ints, pk=pk), ex, dev, need_values=False,
                        ctx=object(), world_size=2)
    # a mapping is checked like a ColumnarData
    with pytest.raises(ValueError, match="n_partitions"):
        columnar.encode({"pid": ints, "pk": pk, "n_partitions": 2}, ex, dev, need_values=False,
                        ctx=object())


def test_host_hash_equals_the_reference():
    rng = np.random.default_rng(5)
    raw = [w.encode("utf-8") for w in WORDS]
    raw += [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 40, 500)]
    raw.append(bytes(rng.integers(0, 256, 5000, dtype=np.uint8)))
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in raw])]).astype(np.int64)
    data = np.frombuffer(b"".join(raw), dtype=np.uint8)
    for seed in (0, 1, (1 << 64) - 3):
        col = StringColumn(offsets, data, hash_seed=seed)
        got = distributed.string_key_hash(col)
        assert got.dtype == torch.int64
        assert np.array_equal(got.numpy(), string_ref.keys(raw, seed))
    # the empty string's key is fmix64(seed); the length enters every key
    assert string_ref.key(b"", 0) == 0 and string_ref.key(b"\0", 0) != string_ref.key(b"\0\0", 0)
    a = distributed.string_key_hash(StringColumn(offsets, data)).numpy()
    b = distributed.string_key_hash(StringColumn(offsets, data, hash_seed=9)).numpy()
    assert not np.any(a == b)


def test_host_hash_counts_invalid_offsets():
    data = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    offsets = np.array([0, 3, 2, 9, 8], dtype=np.int64)  # b"abc", end < start, end > len, ...
    keys, bad = string_columns.host_keys(offsets, data)
    assert bad == 3 and keys[0] == string_ref.keys([b"abc"])[0]
    assert keys[1] == keys[2] == keys[3] == 0
    keys, bad = string_columns.host_keys(np.array([-1, 2, 4], dtype=np.int64), data)
    assert bad == 1 and keys[0] == 0 and keys[1] == string_ref.keys([b"cd"])[0]
