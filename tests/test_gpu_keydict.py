"""The key dictionary kernels through the C ABI against numpy: the set
dpg_keydict_keys lists equals np.unique of the inserted records, after
dpg_keydict_assign every record's dpg_keydict_lookup is its key's id, absent
and reserved keys give -1 and are counted.  Shapes: the wave and block tails,
one key a hundred thousand times, load factors 0.38 and 0.76, a thousand keys
sharing one home slot three slots before the table's end (the chain wraps), the
extreme key values, a table that is too small (the call returns and reports
it), and two inserts into one table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    assert _native.KEYDICT_EMPTY == 1 << 63
    c = _native.Context(0, 11)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


class Table:
    def __init__(self, ctx, capacity):
        self.ctx, self.capacity = ctx, capacity
        self.slots = torch.full((capacity,), I64_MIN, dtype=torch.int64, device="cuda")
        self.slot_ids = torch.full((capacity,), -7, dtype=torch.int32, device="cuda")
        self.info = torch.zeros(2, dtype=torch.int64, device="cuda")

    def insert(self, keys):
        d = _dev(keys)
        self.ctx.keydict_insert(d.data_ptr(), d.numel(), self.slots.data_ptr(), self.capacity,
                                self.info.data_ptr(), None)

    def keys(self):
        out = torch.full((self.capacity,), 12345, dtype=torch.int64, device="cuda")
        n = torch.full((1,), -9, dtype=torch.int64, device="cuda")
        self.ctx.keydict_keys(self.slots.data_ptr(), self.capacity, out.data_ptr(), n.data_ptr(),
                              None)
        k = int(n.item())
        assert (out[k:] == 12345).all()  # nothing is written past the count
        return out[:k].cpu().numpy()

    def assign(self, keys, ids):
        dk, di = _dev(keys), _dev(ids)
        miss = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.ctx.keydict_assign(dk.data_ptr(), di.data_ptr(), dk.numel(), self.slots.data_ptr(),
                                self.slot_ids.data_ptr(), self.capacity, miss.data_ptr(), None)
        return int(miss.item())

    def lookup(self, keys):
        d = _dev(keys)
        out = torch.full((max(d.numel(), 1),), 777, dtype=torch.int64, device="cuda")
        miss = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.ctx.keydict_lookup(d.data_ptr(), d.numel(), self.slots.data_ptr(),
                                self.slot_ids.data_ptr(), self.capacity, out.data_ptr(),
                                miss.data_ptr(), None)
        return out[:d.numel()].cpu().numpy(), int(miss.item())


def _check(ctx, batches, capacity):
    """Inserts the batches into one table and checks every call against numpy."""
    t = Table(ctx, capacity)
    for b in batches:
        t.insert(b)
    records = (np.concatenate(batches) if batches else np.zeros(0)).astype(np.int64)
    reserved = records == I64_MIN
    want = np.unique(records[~reserved])
    got = t.keys()
    info = t.info.tolist()
    assert info == [int(reserved.sum()), 0]
    assert np.array_equal(np.sort(got), want)
    # ids that are neither positions nor sorted ranks; the largest id allowed among them
    ids = (np.arange(len(got), dtype=np.int64) * 3 + 5) % ((1 << 32) - 1)
    if len(ids):
        ids[0] = (1 << 32) - 2
    assert t.assign(got, ids) == 0
    order = np.argsort(got)
    want_ids = np.where(reserved, -1, ids[order][np.searchsorted(want, records).clip(
        max=max(len(want) - 1, 0))] if len(want) else -1)
    out, miss = t.lookup(records)
    assert np.array_equal(out, want_ids)
    assert miss == int(reserved.sum())
    # keys that were never inserted, and the reserved key
    rng = np.random.default_rng(5)
    absent = rng.integers(I64_MIN + 1, I64_MAX, 300, dtype=np.int64)
    absent = absent[~np.isin(absent, want)]
    probe = np.concatenate([absent, [I64_MIN], want[:10]])
    out, miss = t.lookup(probe)
    assert (out[:len(absent) + 1] == -1).all() and miss == len(absent) + 1
    assert np.array_equal(out[len(absent) + 1:], ids[order][:len(want[:10])])
    # assigning an absent key is counted and touches nothing
    before = t.slot_ids.clone()
    assert t.assign(np.concatenate([absent[:5], [I64_MIN]]), np.arange(6)) == 6
    assert torch.equal(before, t.slot_ids)
    return t


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_wave_and_block_tails(ctx, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(I64_MIN + 1, I64_MAX, n, dtype=np.int64)
    _check(ctx, [keys] if n else [], 1024)
    # with duplicates: n records over at most 7 keys
    _check(ctx, [keys[rng.integers(0, min(n, 7), n)]] if n else [np.zeros(0, np.int64)], 64)


def test_one_key_many_records(ctx):
    t = _check(ctx, [np.full(100_000, -0x0123456789ABCDEF, np.int64)], 64)
    assert int((t.slots != I64_MIN).sum()) == 1


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
    t = _check(ctx, [np.repeat(keys, 3)], capacity)
    # one chain from the home slot through the end of the table to its start
    occ = (t.slots != I64_MIN).cpu().numpy()
    assert occ[home:].all() and occ[:1000 - 3].all() and occ.sum() == 1000


def test_extreme_and_reserved_keys(ctx):
    keys = np.array([0, -1, 1, I64_MAX, I64_MIN + 1, I64_MIN, I64_MAX - 1, I64_MIN, 0, I64_MIN,
                     1 << 32, -(1 << 32), (1 << 31) - 1], dtype=np.int64)
    t = _check(ctx, [keys], 64)
    assert t.info.tolist() == [3, 0]


def test_full_table_returns_and_reports(ctx):
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(I64_MIN + 1, I64_MAX, 250, dtype=np.int64))[:200]
    records = np.repeat(keys, 2)
    t = Table(ctx, 64)
    t.insert(records)
    reserved, lost = t.info.tolist()
    listed = t.keys()
    assert reserved == 0 and lost > 0
    # the table is full of keys of the input, each once
    assert len(listed) == 64 and len(np.unique(listed)) == 64 and np.isin(listed, keys).all()
    # a record is lost exactly when its key is not in the table
    assert lost == int((~np.isin(records, listed)).sum())
    ids = np.arange(64, dtype=np.int64) + 1000
    assert t.assign(listed, ids) == 0
    out, miss = t.lookup(listed)
    assert np.array_equal(out, ids) and miss == 0
    # lookups of the keys that found no slot end too (a full table has no empty slot)
    rest = keys[~np.isin(keys, listed)]
    out, miss = t.lookup(rest)
    assert (out == -1).all() and miss == len(rest) == 136


def test_two_inserts_into_one_table(ctx):
    rng = np.random.default_rng(8)
    a = rng.integers(-1000, 1000, 5000).astype(np.int64)
    b = np.concatenate([rng.integers(500, 3000, 5000), [I64_MIN]]).astype(np.int64)
    _check(ctx, [a, b, a[:0]], 8192)


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.handle
    buf = torch.full((128,), 7, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    for cap in (0, 32, 63, 96, 2**31 + 64, 2**32, -64):
        assert lib.dpg_keydict_insert(h, p, 4, p, cap, p, None) == INVALID
        assert lib.dpg_keydict_keys(h, p, cap, p, p, None) == INVALID
        assert lib.dpg_keydict_assign(h, p, p, 4, p, p, cap, p, None) == INVALID
        assert lib.dpg_keydict_lookup(h, p, 4, p, p, cap, p, p, None) == INVALID
    assert lib.dpg_keydict_insert(h, p, -1, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_insert(h, None, 4, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_insert(h, p, 4, None, 64, p, None) == INVALID
    assert lib.dpg_keydict_insert(h, p, 4, p, 64, None, None) == INVALID
    assert lib.dpg_keydict_insert(h, p, 2**31, p, 64, p, None) == UNSUPPORTED
    assert lib.dpg_keydict_keys(h, None, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_keys(h, p, 64, None, p, None) == INVALID
    assert lib.dpg_keydict_keys(h, p, 64, p, None, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, p, -1, p, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_assign(h, None, p, 4, p, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, None, 4, p, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, p, 4, None, p, 64, p, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, p, 4, p, None, 64, p, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, p, 4, p, p, 64, None, None) == INVALID
    assert lib.dpg_keydict_assign(h, p, p, 2**31, p, p, 64, p, None) == UNSUPPORTED
    assert lib.dpg_keydict_lookup(h, p, -1, p, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_lookup(h, None, 4, p, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_lookup(h, p, 4, None, p, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_lookup(h, p, 4, p, None, 64, p, p, None) == INVALID
    assert lib.dpg_keydict_lookup(h, p, 4, p, p, 64, None, p, None) == INVALID
    assert lib.dpg_keydict_lookup(h, p, 4, p, p, 64, p, None, None) == INVALID
    assert lib.dpg_keydict_lookup(h, p, 2**31, p, p, 64, p, p, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 7).all()  # the device was not touched
