"""dpg_keydict_insert_slots and dpg_keydict_gather_ids through the C ABI against
numpy.  After the inserts every stored record's slot holds its key, equal keys
have equal slots, the occupied set is np.unique of the records, and reserved
and lost records carry the sentinel and are counted; which slot a key gets
depends on the arrival order and is not pinned.  The gather equals
slot_ids[out_slots], with -1 and the count for sentinels.  Shapes: the wave and
block tails, one key a hundred thousand times, load factors 0.38 and 0.76, a
thousand keys sharing one home slot three slots before the table's end (the
chain wraps), the extreme key values, the reserved key, a full table, and two
inserts into one table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NO_SLOT = 0xFFFFFFFF
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    assert _native.KEYDICT_NO_SLOT == NO_SLOT
    c = _native.Context(0, 13)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


class Table:
    def __init__(self, ctx, capacity):
        self.ctx, self.capacity = ctx, capacity
        self.slots = torch.full((capacity,), I64_MIN, dtype=torch.int64, device="cuda")
        self.info = torch.zeros(2, dtype=torch.int64, device="cuda")

    def insert(self, keys):
        """The records' slots as uint32 values (int64 numpy)."""
        d = _dev(keys)
        n = d.numel()
        out = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.ctx.keydict_insert_slots(d.data_ptr(), n, self.slots.data_ptr(), self.capacity,
                                      out.data_ptr(), self.info.data_ptr(), None)
        assert (out[n:] == 0x5A5A5A5A).all()  # nothing is written past the records
        return out[:n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF

    def gather(self, rec_slots, slot_ids):
        s = torch.from_numpy((rec_slots & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
        ids = torch.from_numpy(np.ascontiguousarray(slot_ids, dtype=np.uint32)
                               .view(np.int32)).cuda()
        assert ids.numel() == self.capacity
        n = s.numel()
        out = torch.full((n + 8,), 777, dtype=torch.int64, device="cuda")
        miss = torch.full((1,), 100, dtype=torch.int64, device="cuda")
        self.ctx.keydict_gather_ids(s.data_ptr(), n, ids.data_ptr(), self.capacity,
                                    out.data_ptr(), miss.data_ptr(), None)
        assert (out[n:] == 777).all()
        return out[:n].cpu().numpy(), int(miss.item()) - 100  # the counter is added to


def _check(ctx, batches, capacity, lost_ok=False):
    """Inserts the batches into one table; checks slots, counters and the gather."""
    t = Table(ctx, capacity)
    got = [t.insert(b) for b in batches]
    records = np.concatenate([np.asarray(b, dtype=np.int64) for b in batches])
    rec_slots = np.concatenate(got)
    table = t.slots.cpu().numpy()
    reserved = records == I64_MIN
    stored = rec_slots != NO_SLOT
    n_reserved, n_lost = t.info.tolist()
    assert n_reserved == int(reserved.sum())
    assert not stored[reserved].any()
    assert n_lost == int((~stored & ~reserved).sum())
    if not lost_ok:
        assert n_lost == 0
    # every stored record's slot holds its key: equal keys then have equal
    # slots, a slot holding one key
    assert (rec_slots[stored] < capacity).all()
    assert np.array_equal(table[rec_slots[stored]], records[stored])
    # the occupied set
    occupied = np.sort(table[table != I64_MIN])
    assert len(np.unique(occupied)) == len(occupied)
    if lost_ok:
        assert np.array_equal(occupied, np.unique(records[stored]))
        # a record is lost exactly when its key is not in the table
        assert np.array_equal(~stored & ~reserved, ~np.isin(records, occupied) & ~reserved)
    else:
        assert np.array_equal(occupied, np.unique(records[~reserved]))
    # the gather: ids that are neither slots nor ranks, the largest uint32 among them
    slot_ids = (np.arange(capacity, dtype=np.uint64) * 2654435761 + 12345) % (1 << 32)
    slot_ids[rec_slots[stored][:1]] = (1 << 32) - 1
    out, miss = t.gather(rec_slots, slot_ids)
    want = np.where(stored, slot_ids[np.where(stored, rec_slots, 0)].astype(np.int64), -1)
    assert np.array_equal(out, want)
    assert miss == int((~stored).sum())
    return t, rec_slots


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_tails(ctx, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(I64_MIN + 1, I64_MAX, n, dtype=np.int64)
    _check(ctx, [keys], 1024)
    # with duplicates: n records over at most 7 keys
    _check(ctx, [keys[rng.integers(0, min(n, 7), n)]], 64)


def test_no_records(ctx):
    t = Table(ctx, 64)
    assert t.insert(np.zeros(0, np.int64)).size == 0
    out, miss = t.gather(np.zeros(0, np.int64), np.zeros(64, np.uint32))
    assert out.size == 0 and miss == 0
    assert t.info.tolist() == [0, 0] and (t.slots == I64_MIN).all()


def test_one_key_many_records(ctx):
    t, rec_slots = _check(ctx, [np.full(100_000, -0x0123456789ABCDEF, np.int64)], 64)
    assert int((t.slots != I64_MIN).sum()) == 1 and len(np.unique(rec_slots)) == 1


@pytest.mark.parametrize("capacity", [131_072, 65_536])
def test_distinct_keys_and_long_chains(ctx, capacity):
    rng = np.random.default_rng(capacity)
    keys = np.unique(rng.integers(I64_MIN + 1, I64_MAX, 50_100, dtype=np.int64))[:50_000]
    assert len(keys) == 50_000
    rng.shuffle(keys)
    # every key twice, the copies far apart
    _check(ctx, [np.concatenate([keys, keys[::-1]])], capacity)


def test_shared_home_slot_wraps_around(ctx):
    from pipelinedp_amd import distributed
    capacity, home = 4096, 4096 - 3
    rng = np.random.default_rng(77)
    cand = torch.from_numpy(rng.integers(I64_MIN + 1, I64_MAX, 6_000_000, dtype=np.int64))
    hit = cand[(distributed.key_hash(cand) & (capacity - 1)) == home].numpy()
    keys = np.unique(hit)[:1000]
    assert len(keys) == 1000
    t, rec_slots = _check(ctx, [np.repeat(keys, 3)], capacity)
    # one chain from the home slot through the end of the table to its start
    occ = (t.slots != I64_MIN).cpu().numpy()
    assert occ[home:].all() and occ[:1000 - 3].all() and occ.sum() == 1000
    assert set(rec_slots.tolist()) == set(range(home, capacity)) | set(range(1000 - 3))


def test_extreme_and_reserved_keys(ctx):
    keys = np.array([0, -1, 1, I64_MAX, I64_MIN + 1, I64_MIN, I64_MAX - 1, I64_MIN, 0, I64_MIN,
                     1 << 32, -(1 << 32), (1 << 31) - 1], dtype=np.int64)
    t, rec_slots = _check(ctx, [keys], 64)
    assert t.info.tolist() == [3, 0]
    assert (rec_slots[keys == I64_MIN] == NO_SLOT).all() and rec_slots[0] == rec_slots[8]


def test_full_table_returns_and_reports(ctx):
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(I64_MIN + 1, I64_MAX, 250, dtype=np.int64))[:200]
    t, rec_slots = _check(ctx, [np.repeat(keys, 2)], 64, lost_ok=True)
    # the table is full; the 136 keys that found no slot lost both their records
    assert int((t.slots != I64_MIN).sum()) == 64
    assert t.info.tolist() == [0, 2 * 136] and int((rec_slots == NO_SLOT).sum()) == 2 * 136


def test_two_inserts_into_one_table(ctx):
    rng = np.random.default_rng(8)
    a = rng.integers(-1000, 1000, 5000).astype(np.int64)
    b = np.concatenate([rng.integers(500, 3000, 5000), [I64_MIN]]).astype(np.int64)
    _check(ctx, [a, b, a[:0]], 8192)


def test_slots_agree_with_plain_insert_and_lookup(ctx):
    """A table filled by dpg_keydict_insert_slots is a table of the four
    existing calls: dpg_keydict_assign and dpg_keydict_lookup on it give what
    the gather gives."""
    rng = np.random.default_rng(21)
    records = rng.integers(-(1 << 62), 1 << 62, 3000, dtype=np.int64)[rng.integers(0, 3000, 20_000)]
    t, rec_slots = _check(ctx, [records], 8192)
    uniq = np.unique(records)
    dk, di = _dev(uniq), _dev(np.arange(len(uniq)))
    slot_ids = torch.zeros(8192, dtype=torch.int32, device="cuda")
    miss = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.keydict_assign(dk.data_ptr(), di.data_ptr(), len(uniq), t.slots.data_ptr(),
                       slot_ids.data_ptr(), 8192, miss.data_ptr(), None)
    d = _dev(records)
    looked = torch.empty(len(records), dtype=torch.int64, device="cuda")
    ctx.keydict_lookup(d.data_ptr(), len(records), t.slots.data_ptr(), slot_ids.data_ptr(), 8192,
                       looked.data_ptr(), miss.data_ptr(), None)
    out, gmiss = t.gather(rec_slots, slot_ids.cpu().numpy().view(np.uint32))
    assert int(miss.item()) == 0 and gmiss == 0
    assert np.array_equal(out, looked.cpu().numpy())
    assert np.array_equal(out, np.searchsorted(uniq, records))


def test_gather_treats_any_non_slot_as_missing(ctx):
    """Only 0xFFFFFFFF is written by the insert, but no value at or above the
    capacity is ever used as an index."""
    t = Table(ctx, 64)
    slot_ids = np.arange(64, dtype=np.uint32) + 500
    rec = np.array([0, 63, 64, 1 << 31, NO_SLOT, 5], dtype=np.int64)
    out, miss = t.gather(rec, slot_ids)
    assert out.tolist() == [500, 563, -1, -1, -1, 505] and miss == 3


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = torch.full((128,), 7, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    for cap in (0, 32, 63, 96, 2**31 + 64, 2**32, -64):
        assert lib.dpg_keydict_insert_slots(h, p, 4, p, cap, p, p, None) == INVALID
        assert lib.dpg_keydict_gather_ids(h, p, 4, p, cap, p, p, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, p, -1, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, None, 4, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, p, 4, None, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, p, 4, p, 64, None, p, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, p, 4, p, 64, p, None, None) == INVALID
    assert lib.dpg_keydict_insert_slots(h, p, 2**31, p, 64, p, p, None) == UNSUPPORTED
    assert lib.dpg_keydict_gather_ids(h, p, -1, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_gather_ids(h, None, 4, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_gather_ids(h, p, 4, None, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_gather_ids(h, p, 4, p, 64, None, p, None) == INVALID
    assert lib.dpg_keydict_gather_ids(h, p, 4, p, 64, p, None, None) == INVALID
    assert lib.dpg_keydict_gather_ids(h, p, 2**31, p, 64, p, p, None) == UNSUPPORTED
    # n == 0 is a no-op: the per-record pointers may be NULL
    assert lib.dpg_keydict_insert_slots(h, None, 0, p, 64, None, p, None) == 0
    assert lib.dpg_keydict_gather_ids(h, None, 0, p, 64, None, p, None) == 0
    torch.cuda.synchronize()
    assert (buf == 7).all()  # the device was not touched
