"""distributed.build_string_dictionary on host columns: in one process and over
gloo (world 2 and 3).  The host path runs the protocol of the device path --
the same collectives, splits, ids and error agreement -- with numpy
restatements of the kernels, so all of that is checked without a GPU.

2 000 records over 120 strings ('' , non-ASCII and one of 200 bytes among
them), dealt round-robin.  The ids must be exactly i * R + owner, computed here
from tests/string_ref.py hashes (tests/string_pack_ref.py: global_ids)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import string_pack_ref, string_ref

N, N_STR = 2_000, 120
SEED = 11
WORLDS = [1, 2, 3]
CONSTANT_KEY = 0x1234_5678_9ABC


def _strings():
    s = [f"key-{i:03d}/{'x' * (i % 23)}" for i in range(N_STR)]
    s[0], s[1], s[2], s[3] = "", "é", "日本語 テキスト", "\U00010000 astral"
    s[4] = "long " + "0123456789" * 19 + "tail!"  # 200 bytes
    assert len(s[4].encode()) == 200 and len(set(s)) == N_STR
    return s


def _public():
    """20 strings of the data and 6 that no record holds."""
    return _strings()[::6] + [f"absent/{i}" for i in range(5)] + ["абсент"]


def _records():
    rng = np.random.default_rng(2024)
    idx = rng.integers(0, N_STR, N)
    idx[:N_STR] = np.arange(N_STR)  # every string occurs
    strings = _strings()
    return [strings[i] for i in idx]


def _local(world, rank, case):
    rec = _records()
    if case == "collision":
        return [["alpha"] * 5, ["beta"] * 3, []][rank]
    if case == "empty" and rank == world - 1:
        return []
    if case == "overflow" and rank > 0:
        return [r for r in rec[rank::world] if r in _strings()[:30]]
    if case == "overflow":
        return rec
    return rec[rank::world]


def _build(world, rank, case, group):
    import pipelinedp_amd as pdp
    from pipelinedp_amd import distributed, string_columns
    col = pdp.StringColumn.from_strings(_local(world, rank, case), hash_seed=SEED)
    if case == "bad_offsets" and rank == 0:
        col.offsets[5] = -1  # records 4 and 5
    if case == "collision":
        string_columns.host_keys = lambda off, data, seed=0: (
            np.full(len(off) - 1, CONSTANT_KEY, dtype=np.int64), 0)
    public = _public() if case in ("public", "empty") else None
    try:
        sd = distributed.build_string_dictionary(
            col, public, group, max_distinct=20 if case == "overflow" else None)
    except (ValueError, RuntimeError) as e:
        return (type(e).__name__, str(e))
    table = sd.strings(torch.arange(sd.owned_keys.numel()))
    return ("ok", sd.ids.numpy(), None if sd.public_ids is None else sd.public_ids.numpy(),
            sd.n_partitions, sd.owned_keys.numpy(), table)


def _worker(rank, world, port, case, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _build(world, rank, case, dist.group.WORLD)))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, case):
    """[rank] -> what _build returned.  A rank that hangs in a collective the
    others left fails the q.get / join time-outs."""
    if world == 1:
        return [_build(1, 0, case, None)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=90) for _ in range(world)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return [out for _, out in res]


def _check(world, case, res, with_public):
    universe = set(_strings()) | (set(_public()) if with_public else set())
    want_ids, want_P = string_pack_ref.global_ids(universe, world, SEED)
    tables = []
    for rank, out in enumerate(res):
        assert out[0] == "ok", out
        _, ids, public_ids, P, owned_keys, table = out
        local = _local(world, rank, case)
        assert ids.dtype == np.int64
        assert np.array_equal(ids, np.array([want_ids[s] for s in local], dtype=np.int64))
        assert P == want_P
        if with_public:
            assert np.array_equal(public_ids, np.array([want_ids[s] for s in _public()]))
        else:
            assert public_ids is None
        # the owned table: this owner's strings in ascending signed hash order
        assert table == string_pack_ref.owned_strings(universe, world, rank, SEED)
        assert np.array_equal(owned_keys, string_ref.keys([s.encode() for s in table], SEED))
        assert np.array_equal(owned_keys, np.sort(owned_keys))
        for i, s in enumerate(table):
            assert want_ids[s] == i * world + rank
        tables.append(table)
    flat = [s for t in tables for s in t]
    assert len(flat) == len(set(flat)) and set(flat) == universe  # disjoint, and the union


@pytest.mark.parametrize("world", WORLDS)
def test_ids_are_hash_ranks_per_owner(world):
    _check(world, "plain", _run(world, "plain"), with_public=False)


@pytest.mark.parametrize("world", WORLDS)
def test_public_strings_absent_from_the_data_get_ids(world):
    res = _run(world, "public")
    _check(world, "public", res, with_public=True)
    want_ids, _ = string_pack_ref.global_ids(set(_strings()) | set(_public()), world, SEED)
    absent = [s for s in _public() if s not in set(_strings())]
    assert len(absent) == 6
    for out in res:
        got = dict(zip(_public(), out[2].tolist()))
        assert all(got[s] == want_ids[s] for s in absent)


@pytest.mark.parametrize("world", [2, 3])
def test_rank_without_records(world):
    res = _run(world, "empty")
    assert res[world - 1][1].size == 0
    _check(world, "empty", res, with_public=True)


@pytest.mark.parametrize("world", [2, 3])
def test_collision_across_ranks_raises_on_every_rank(world):
    """One constant key for every string; rank 0 holds only 'alpha' and rank 1
    only 'beta', so each rank's local check is clean and only the key's owner
    sees two strings under it."""
    res = _run(world, "collision")
    want = ("ValueError", "1 records or strings share a 64-bit hash with a different string; "
                          "pass another hash_seed")
    assert res == [want] * world


@pytest.mark.parametrize("world", WORLDS)
def test_invalid_offsets_on_one_rank_raise_on_every_rank(world):
    res = _run(world, "bad_offsets")
    want = ("ValueError", "2 records of the partition key StringColumn have offsets outside "
                          "0 <= offsets[i] <= offsets[i + 1] <= len(data)")
    assert res == [want] * world


@pytest.mark.parametrize("world", WORLDS)
def test_table_overflow_on_one_rank_raises_on_every_rank(world):
    """max_distinct_partition_keys=20 gives a table of 64 slots: rank 0 holds
    all 120 strings, the other ranks at most 30."""
    rec = _local(world, 0, "overflow")
    seen = list(dict.fromkeys(rec))
    lost = sum(1 for r in rec if r in set(seen[64:]))
    assert len(seen) == N_STR and lost > 0
    res = _run(world, "overflow")
    for out in res:
        assert out[0] == "ValueError", out
        assert out[1].startswith(
            f"string partition keys: the key table sized by max_distinct_partition_keys=20 "
            f"overflowed ({lost} records found no slot)")
    assert all(out == res[0] for out in res)


def test_host_restatements_equal_the_reference():
    """string_columns.host_pack / host_verify_runs against tests/string_pack_ref."""
    from pipelinedp_amd import string_columns
    import pipelinedp_amd as pdp
    strings = _strings()[:40]
    col = pdp.StringColumn.from_strings(strings)
    offsets, data = col.host_columns()
    offsets = offsets.copy()
    offsets[8] = offsets[9] + 1  # records 7 and 8 invalid
    rng = np.random.default_rng(5)
    records = np.concatenate([rng.integers(0, 40, 100), [-1, 40, 7, 8]])
    oo, od, bad = string_columns.host_pack(offsets, data, records)
    want_len, want_bad = string_pack_ref.lengths(offsets, data.size, 40, records)
    assert bad == want_bad == 4
    assert np.array_equal(np.diff(oo), want_len) and oo[0] == 0
    out = bytearray(int(oo[-1]))
    assert string_pack_ref.pack(offsets, data.tobytes(), 40, records, oo, out) == 4
    assert bytes(out) == od.tobytes()
    keys = np.array([5, 5, 5, 6, 7, 7, 7, 7], dtype=np.int64)
    order = np.array([3, 3, 4, 9, 0, 0, 8, 8], dtype=np.uint32)
    got = string_columns.host_verify_runs(keys, order, offsets, data)
    want = string_pack_ref.verify_runs(keys, order, offsets, data.tobytes(), 40)
    assert (got[0].tolist(), got[1], got[2]) == want == ([1, 0, 0, 1, 1, 0, 0, 0], 3, 2)


def test_flag_needs_a_string_column():
    import pipelinedp_amd as pdp
    c = pdp.ColumnarData(pk=pdp.StringColumn.from_strings(["a"]), global_string_keys=True)
    assert c.global_string_keys is True
    assert pdp.ColumnarData(pk=[1, 2]).global_string_keys is False
    with pytest.raises(ValueError, match="global_string_keys=True .* pk must be a StringColumn"):
        pdp.ColumnarData(pk=torch.tensor([1, 2]), global_string_keys=True)
    with pytest.raises(ValueError, match="pk must be a StringColumn"):
        pdp.ColumnarData(pk=["a", "b"], global_string_keys=True)
    with pytest.raises(ValueError, match="n_partitions must not be given"):
        pdp.ColumnarData(pk=pdp.StringColumn.from_strings(["a"]), n_partitions=3,
                         global_string_keys=True)
    with pytest.raises(ValueError, match="sparse_partition_keys"):
        pdp.ColumnarData(pk=pdp.StringColumn.from_strings(["a"]), sparse_partition_keys=True,
                         global_string_keys=True)
