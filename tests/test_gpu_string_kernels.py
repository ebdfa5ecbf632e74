"""dpg_string_hash, dpg_keydict_representatives and dpg_string_verify at the
ABI level, against tests/string_ref.py and numpy."""
import ctypes

import numpy as np
import pytest
import torch

from tests import string_ref

N_HASH = 300_000  # more than one pass of the grid (n_cu * 8 blocks of 256 lanes)
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    """300 000 strings (one of 5 000 bytes, in the middle), their column and
    their reference keys under seed 0; shared, never modified."""
    rng = np.random.default_rng(18)
    lens = np.asarray(LENGTHS)[rng.integers(0, len(LENGTHS), N_HASH)]
    lens[N_HASH // 2] = 5000
    lens[-1] = 17  # the last record ends exactly at data_len, on no word boundary
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    return offsets, data, string_ref.keys_of_column(offsets, data, 0)


def _sptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hash(ctx, offsets_t, data_t, seed=0):
    n = offsets_t.numel() - 1
    keys = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    info = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.string_hash(offsets_t.data_ptr(), data_t.data_ptr(), data_t.numel(), n, seed,
                    keys.data_ptr(), info.data_ptr(), _sptr())
    return keys.cpu().numpy(), int(info.item())


@pytest.mark.gpu
def test_hash_equals_reference(ctx, corpus):
    offsets, data, want = corpus
    got, bad = _hash(ctx, torch.from_numpy(offsets).cuda(), torch.from_numpy(data).cuda())
    assert bad == 0
    assert np.array_equal(got, want)
    assert int(offsets[-1]) == data.size  # nothing behind the last record


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_hash_of_a_misaligned_slice(ctx, corpus, k):
    """data = big[k:k + len] inside a buffer of 0xFF: a misaligned base, and
    neighbouring bytes that must not enter the first or the last hash."""
    offsets, data, want = corpus
    big = torch.full((data.size + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    big[k:k + data.size] = torch.from_numpy(data).cuda()
    view = big[k:k + data.size]
    assert view.data_ptr() % 8 == k
    got, bad = _hash(ctx, torch.from_numpy(offsets).cuda(), view)
    assert bad == 0
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_hash_counts_invalid_offsets(ctx):
    raw = [b"alpha", b"", b"0123456789abcdefg", b"tail"]
    data = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    L = data.size
    #          alpha  neg     ok("")  end<start  ok(17)  end>len   ok: data[22:26] = b"tail"
    starts = [0,      -3,     5,      9,         5,      20,       22]
    ends = [5,        2,      5,      8,         22,     L + 1,    L]
    # a column whose records are (starts[i], ends[i]): one call per record pair
    # is not needed -- offsets need not be monotone for the call, only per record
    got, bad_total = [], 0
    for a, b in zip(starts, ends):
        k, bad = _hash(ctx, torch.tensor([a, b], dtype=torch.int64, device="cuda"),
                       torch.from_numpy(data).cuda())
        got.append(int(k[0]))
        bad_total += bad
    buf = data.tobytes()
    valid = [0, 2, 4, 6]
    assert bad_total == 3
    for i in range(len(starts)):
        if i in valid:
            assert got[i] == int(string_ref.keys([buf[starts[i]:ends[i]]])[0])
        else:
            assert got[i] == 0
    # in one column: invalid records beside valid ones
    offsets = np.array([0, 5, 5, 22, 21, L + 1, L - 4, L], dtype=np.int64)
    keys, bad = _hash(ctx, torch.from_numpy(offsets).cuda(), torch.from_numpy(data).cuda())
    ok = [0, 1, 2, 6]  # (22, 21): end < start; (21, L + 1), (L + 1, L - 4): past the data
    assert bad == 3
    for i in range(7):
        a, b = int(offsets[i]), int(offsets[i + 1])
        assert keys[i] == (string_ref.keys([buf[a:b]])[0] if i in ok else 0)
    neg = np.array([-1, 4], dtype=np.int64)
    keys, bad = _hash(ctx, torch.from_numpy(neg).cuda(), torch.from_numpy(data).cuda())
    assert bad == 1 and keys[0] == 0


@pytest.mark.gpu
def test_hash_of_nothing_and_bad_arguments(ctx):
    from pipelinedp_amd import _native
    keys, bad = _hash(ctx, torch.zeros(1, dtype=torch.int64, device="cuda"),
                      torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert keys.size == 0 and bad == 0
    # counters are added to
    off = torch.tensor([0, 2, 1], dtype=torch.int64, device="cuda")
    data = torch.zeros(2, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.int64, device="cuda")
    info = torch.full((1,), 40, dtype=torch.int64, device="cuda")
    ctx.string_hash(off.data_ptr(), data.data_ptr(), 2, 2, 0, out.data_ptr(), info.data_ptr(),
                    _sptr())
    assert int(info.item()) == 41
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.string_hash(off.data_ptr(), data.data_ptr(), 2, 2, 0, out.data_ptr(), None, _sptr())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.string_hash(off.data_ptr(), data.data_ptr(), -1, 2, 0, out.data_ptr(),
                        info.data_ptr(), _sptr())
    with pytest.raises(_native.NativeError, match="unsupported"):
        ctx.string_hash(off.data_ptr(), data.data_ptr(), 2, 1 << 31, 0, out.data_ptr(),
                        info.data_ptr(), _sptr())
    rep = torch.empty(64, dtype=torch.int32, device="cuda")
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.keydict_representatives(rep.data_ptr(), 2, 48, rep.data_ptr(), _sptr())
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.string_verify(off.data_ptr(), data.data_ptr(), 2, 2, rep.data_ptr(), None,
                          info.data_ptr(), _sptr())


@pytest.mark.gpu
def test_a_seed_changes_every_key(ctx, corpus):
    offsets, data, want = corpus
    n = 4096
    off = torch.from_numpy(offsets[:n + 1]).cuda()
    dat = torch.from_numpy(data[:int(offsets[n])]).cuda()
    seed = 0xFEEDFACECAFEBEEF
    got, _ = _hash(ctx, off, dat, seed)
    assert np.array_equal(got, string_ref.keys_of_column(offsets[:n + 1], data, seed))
    assert not np.any(got == want[:n])


def _representatives(ctx, rec_slots: np.ndarray, capacity: int):
    slots_t = torch.from_numpy(rec_slots.astype(np.uint32).view(np.int32)).cuda()
    rep = torch.full((capacity,), -1, dtype=torch.int32, device="cuda")
    ctx.keydict_representatives(slots_t.data_ptr(), rec_slots.size, capacity, rep.data_ptr(),
                                _sptr())
    return rep.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [50, 100_000], ids=["hot", "cold"])
def test_representatives_are_first_occurrences(ctx, n_slots):
    rng = np.random.default_rng(n_slots)
    n, capacity = 200_000, 1 << 18
    where = rng.choice(capacity, n_slots, replace=False).astype(np.int64)
    rec = where[rng.integers(0, n_slots, n)]
    rec[rng.integers(0, n, 500)] = NO_SLOT  # records without a slot are skipped
    want = np.full(capacity, NO_SLOT, dtype=np.uint32)
    has = rec != NO_SLOT
    uniq, first = np.unique(rec[has], return_index=True)
    want[uniq] = np.nonzero(has)[0][first]
    assert np.array_equal(_representatives(ctx, rec, capacity), want)
    ctx.keydict_representatives(None, 0, capacity,
                                torch.empty(capacity, dtype=torch.int32, device="cuda").data_ptr(),
                                _sptr())  # n == 0: a no-op


def _verify(ctx, strings, rec_slots, rep, pad=0):
    """The mismatch count for a hand-made column, slots and representatives."""
    raw = b"".join(strings)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    big = torch.full((len(raw) + pad + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    big[pad:pad + len(raw)] = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    data = big[pad:pad + len(raw)]
    slots_t = torch.from_numpy(np.asarray(rec_slots, dtype=np.uint32).view(np.int32)).cuda()
    rep_t = torch.from_numpy(np.asarray(rep, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.string_verify(torch.from_numpy(offsets).cuda().data_ptr(), data.data_ptr(), len(raw),
                      len(strings), slots_t.data_ptr(), rep_t.data_ptr(), out.data_ptr(), _sptr())
    return int(out.item())


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
def test_verify_counts_exactly(ctx, pad):
    base = b"0123456789abcdefghijklmnopqrstuvwxyz!"  # 37 bytes: 4 words and a tail of 5
    strings = [
        base,                       # 0: representative of slot 0
        base[:-1] + b"?",           # 1: same length, last byte differs
        b"#" + base[1:],            # 2: same length, first byte differs
        base[:20],                  # 3: shorter, a common prefix
        base + b"more",             # 4: longer, a common prefix
        base,                       # 5: equal, at another alignment
        b"",                        # 6: representative of slot 1
        b"x",                       # 7: non-empty against empty
        b"",                        # 8: equal to 6
        base[:16],                  # 9: representative of slot 2 (whole words only)
        base[:15] + b"Z",           # 10: differs in the last byte of the last word
        base[:16],                  # 11: equal
        b"no slot, never compared",  # 12
        b"",                        # 13: empty against the non-empty representative 0
    ]
    rec_slots = [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, NO_SLOT, 0]
    rep = [0, 6, 9] + [NO_SLOT] * 61
    assert _verify(ctx, strings, rec_slots, rep, pad) == 7  # records 1, 2, 3, 4, 7, 10, 13
    # all equal: nothing to count
    assert _verify(ctx, [base, b"", base, b"", base], [5, 7, 5, 7, 5],
                   [NO_SLOT] * 5 + [0, NO_SLOT, 1], pad) == 0
    # a slot without a representative counts as a mismatch, and reads nothing
    assert _verify(ctx, [base, base], [0, 3], [0] + [NO_SLOT] * 63, pad) == 1


@pytest.mark.gpu
def test_verify_checks_offsets(ctx):
    data = torch.from_numpy(np.frombuffer(b"abcdabcd", dtype=np.uint8).copy()).cuda()
    # records: "abcd", (4, 3) invalid, (3, 9) past the data, "" -- all in slot 0, rep 0
    offsets = torch.tensor([0, 4, 3, 9, 9], dtype=torch.int64, device="cuda")
    slots_t = torch.zeros(4, dtype=torch.int32, device="cuda")
    rep_t = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.string_verify(offsets.data_ptr(), data.data_ptr(), 8, 4, slots_t.data_ptr(),
                      rep_t.data_ptr(), out.data_ptr(), _sptr())
    assert int(out.item()) == 3  # (9, 9) is past the data too
    # an invalid representative: every record of its slot is a mismatch
    offsets = torch.tensor([5, 2, 4], dtype=torch.int64, device="cuda")
    out.zero_()
    ctx.string_verify(offsets.data_ptr(), data.data_ptr(), 8, 2, slots_t.data_ptr(),
                      rep_t.data_ptr(), out.data_ptr(), _sptr())
    assert int(out.item()) == 2
