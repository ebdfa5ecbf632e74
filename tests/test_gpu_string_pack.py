"""dpg_string_lengths, dpg_string_pack and dpg_string_verify_runs at the ABI
level, against tests/string_pack_ref.py (Python over `bytes`).  All values are
integers and bytes: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import string_pack_ref as ref

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 63, 64, 65)
N_STR = 64
GUARD = 64
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 5  # DPG_OK, DPG_ERR_INVALID_ARG, DPG_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx(built):
    from pipelinedp_amd import _native
    c = _native.Context(0, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    """64 strings of every length in LENGTHS and one of 300 bytes, random bytes
    with 0x00 and 0xFF among them; shared, never modified."""
    rng = np.random.default_rng(19)
    lens = np.asarray(LENGTHS * 6)[:N_STR].copy()
    rng.shuffle(lens)
    lens[N_STR // 2] = 300
    lens[-1] = 17  # the last record ends exactly at data_len, on no word boundary
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    data[::5] = 0x00
    data[2::7] = 0xFF
    assert set(LENGTHS) | {300} == set(lens.tolist())
    return offsets, data


def _sptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _records(m):
    """m record indices: out of order, with repeats, every record when m >= 64."""
    rng = np.random.default_rng(1000 + m)
    r = rng.integers(0, N_STR, m)
    if m >= N_STR:
        r[:N_STR] = rng.permutation(N_STR)
    if m > 1:
        r[-1] = r[0]  # a repeat even in short lists
    return r.astype(np.int64)


def _lengths(ctx, offsets_t, data_len, n, records_t, info=None):
    m = records_t.numel()
    out = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    info = torch.zeros(1, dtype=torch.int64, device="cuda") if info is None else info
    ctx.string_lengths(offsets_t.data_ptr(), data_len, n, records_t.data_ptr(), m, out.data_ptr(),
                       info.data_ptr(), _sptr())
    return out.cpu().numpy(), int(info.item())


def _pack_case(ctx, offsets, data, n, records, out_offsets, k=0):
    """Runs dpg_string_pack with `data` cut out of a buffer of 0xFF at byte k
    and the output cut out of a buffer of 0xEE at byte k behind a guard;
    returns (output bytes, invalid count) and checks guards and source."""
    total = int(out_offsets[-1]) if len(out_offsets) else 0
    src_big = torch.full((data.size + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    src_big[k:k + data.size] = _dev(data)
    src = src_big[k:k + data.size]
    out_big = torch.full((total + 2 * GUARD + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    out = out_big[GUARD + k:GUARD + k + total]
    if k and total:
        assert src.data_ptr() % 8 == k and out.data_ptr() % 8 == k
    src_before = src_big.clone()
    info = torch.zeros(1, dtype=torch.int64, device="cuda")
    off_t, rec_t, oo_t = _dev(offsets), _dev(records), _dev(out_offsets)  # alive over the call
    ctx.string_pack(off_t.data_ptr(), src.data_ptr(), data.size, n, rec_t.data_ptr(),
                    len(records), oo_t.data_ptr(), out.data_ptr(), total, info.data_ptr(),
                    _sptr())
    torch.cuda.synchronize()
    got = out_big.cpu().numpy()
    assert np.all(got[:GUARD + k] == 0xEE) and np.all(got[GUARD + k + total:] == 0xEE)
    assert torch.equal(src_big, src_before)
    return got[GUARD + k:GUARD + k + total].tobytes(), int(info.item())


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3, 5, 7])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_pack_and_lengths_equal_reference(ctx, corpus, m, k):
    offsets, data = corpus
    records = _records(m)
    want_len, want_bad = ref.lengths(offsets, data.size, N_STR, records)
    got_len, bad = _lengths(ctx, _dev(offsets), data.size, N_STR, _dev(records))
    assert bad == want_bad == 0
    assert got_len.tolist() == want_len
    out_offsets = np.concatenate([[0], np.cumsum(want_len)]).astype(np.int64)
    want = bytearray(b"\xEE" * int(out_offsets[-1]))
    assert ref.pack(offsets, data.tobytes(), N_STR, records, out_offsets, want) == 0
    got, bad = _pack_case(ctx, offsets, data, N_STR, records, out_offsets, k)
    assert bad == 0
    assert got == bytes(want)


@pytest.mark.gpu
def test_pack_more_than_one_pass_of_the_grid(ctx, corpus):
    """600 000 records: more than n_cu * 8 blocks of 256 lanes."""
    offsets, data = corpus
    m = 600_000
    records = np.random.default_rng(3).integers(0, N_STR, m).astype(np.int64)
    lens = np.diff(offsets)[records]
    out_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    got_len, bad = _lengths(ctx, _dev(offsets), data.size, N_STR, _dev(records))
    assert bad == 0 and np.array_equal(got_len, lens)
    got, bad = _pack_case(ctx, offsets, data, N_STR, records, out_offsets, 3)
    # the reference, vectorised: byte t of the output is byte (t - out start + start) of data
    which = np.repeat(np.arange(m), lens)
    pos = np.arange(int(out_offsets[-1])) - out_offsets[:-1][which] + offsets[records][which]
    assert bad == 0 and got == data[pos].tobytes()


@pytest.mark.gpu
def test_invalid_entries_are_counted_and_write_nothing(ctx, corpus):
    offsets, data = corpus
    n = N_STR
    bad_off = offsets.copy()
    bad_off[11] = bad_off[10] - 1        # record 10: a descending pair (record 9 stays valid)
    bad_off[41] = data.size + 3          # record 40 ends, record 41 starts past the data
    assert bad_off[12] >= bad_off[11] and bad_off[10] > 0
    #                 -1  n   desc  past  past  then valid neighbours and repeats
    records = np.array([5, -1, 6, n, 10, 9, 40, 41, 11, 39, 42, 5], dtype=np.int64)
    want_len, want_bad = ref.lengths(bad_off, data.size, n, records)
    got_len, bad = _lengths(ctx, _dev(bad_off), data.size, n, _dev(records))
    assert bad == want_bad == 5
    assert got_len.tolist() == want_len
    out_offsets = np.concatenate([[0], np.cumsum(want_len)]).astype(np.int64)
    want = bytearray(b"\xEE" * int(out_offsets[-1]))
    assert ref.pack(bad_off, data.tobytes(), n, records, out_offsets, want) == 5
    got, bad = _pack_case(ctx, bad_off, data, n, records, out_offsets, 1)
    assert bad == 5 and got == bytes(want)
    # an out range that is one byte too short (entry 2); further down one that
    # leaves [0, out_total] (the last entry)
    records = np.array([5, 6, 7, 8, 9, 12, 13, 14], dtype=np.int64)
    lens = np.diff(offsets)[records]
    out_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    short = out_offsets.copy()
    short[3:] -= 1  # entry 2 loses its last byte; the others keep their length
    want = bytearray(b"\xEE" * int(short[-1]))
    assert ref.pack(offsets, data.tobytes(), n, records, short, want) == 1
    got, bad = _pack_case(ctx, offsets, data, n, records, short, 5)
    assert bad == 1 and got == bytes(want)
    assert got[int(short[2]):int(short[3])] == b"\xEE" * int(short[3] - short[2])
    # past out_total: the last entry's range is cut by a smaller out_total
    total = int(out_offsets[-1]) - 1
    out_big = torch.full((total + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    out = out_big[GUARD:GUARD + total]
    info = torch.full((1,), 100, dtype=torch.int64, device="cuda")
    off_t, dat_t, rec_t, oo_t = _dev(offsets), _dev(data), _dev(records), _dev(out_offsets)
    ctx.string_pack(off_t.data_ptr(), dat_t.data_ptr(), data.size, n, rec_t.data_ptr(),
                    len(records), oo_t.data_ptr(), out.data_ptr(), total, info.data_ptr(),
                    _sptr())
    assert int(info.item()) == 101  # added to, not overwritten
    want = bytearray(b"\xEE" * total)
    assert ref.pack(offsets, data.tobytes(), n, records, out_offsets, want) == 1
    got = out_big.cpu().numpy()
    assert got[GUARD:GUARD + total].tobytes() == bytes(want)
    assert np.all(got[:GUARD] == 0xEE) and np.all(got[GUARD + total:] == 0xEE)
    # a column of no records: every index is invalid, nothing is read
    got_len, bad = _lengths(ctx, torch.zeros(1, dtype=torch.int64, device="cuda"), 0, 0,
                            _dev(np.array([0, 1], dtype=np.int64)))
    assert bad == 2 and got_len.tolist() == [0, 0]


def _column(strings):
    lens = [len(s) for s in strings]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offsets, np.frombuffer(b"".join(strings), dtype=np.uint8).copy()


def _verify(ctx, keys, order, offsets, data, n_strings=None, info=None, k=0):
    m = len(keys)
    n_strings = len(offsets) - 1 if n_strings is None else n_strings
    big = torch.full((data.size + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    big[k:k + data.size] = _dev(data)
    head = torch.full((m,), 9, dtype=torch.uint8, device="cuda")
    info = torch.zeros(2, dtype=torch.int64, device="cuda") if info is None else info
    order_t = None if order is None else _dev(np.asarray(order, dtype=np.uint32).view(np.int32))
    keys_t, off_t = _dev(np.asarray(keys, dtype=np.int64)), _dev(offsets)  # alive over the call
    ctx.string_verify_runs(keys_t.data_ptr(), None if order_t is None else order_t.data_ptr(),
                           off_t.data_ptr(), big[k:].data_ptr(), data.size, n_strings, m,
                           head.data_ptr(), info.data_ptr(), _sptr())
    torch.cuda.synchronize()
    return head.cpu().numpy().tolist(), info.cpu().numpy().tolist()


def _verify_corpus():
    """Strings 0-8: one string nine times; then variants of a 20-byte base that
    differ by length, first byte, byte 7, byte 8 and last byte; two empties."""
    base = bytes(range(65, 85))  # 20 bytes
    def flip(i):
        b = bytearray(base)
        b[i] ^= 0x01
        return bytes(b)
    strings = [b"nine times"] * 9 + [base, base, base[:19], flip(0), flip(7), flip(8), flip(19),
                                     b"", b"", base + b"!", b"solo"]
    return strings


@pytest.mark.gpu
def test_verify_runs_heads_and_counts(ctx):
    strings = _verify_corpus()
    offsets, data = _column(strings)
    I64_MIN1 = -(1 << 63) + 1
    # identity order: runs of 9 (equal), 2 (equal), 1, then pairs that differ
    #      0-8: 9 equal | 9,10 equal | 11 alone | 12,13 | 14,15 | 16,17 empties | 18 | 19
    keys = [7] * 9 + [-3, -3] + [I64_MIN1] + [40, 40] + [41, 41] + [0, 0] + [5] + [6]
    want = ref.verify_runs(keys, None, offsets, data.tobytes(), len(strings))
    # (12,13) flip(0) vs flip(7): differ; (14,15) flip(8) vs flip(19): differ; empties equal
    assert want[1:] == (2, 0) and sum(want[0]) == 8
    for k in (0, 3):
        head, info = _verify(ctx, keys, None, offsets, data, k=k)
        assert head == want[0] and info == [2, 0]
    # with an order: runs of length 1, 2, 3 and 9; every kind of mismatch
    #  run A (9): all "nine times"                     -> 0 differences
    #  run B (3): base, base, base[:19]                -> 1 (length)
    #  run C (2): base, flip(0)                        -> 1 (first byte)
    #  run D (2): base, flip(7)                        -> 1 (byte 7)
    #  run E (2): base, flip(8)                        -> 1 (byte 8, the word boundary)
    #  run F (2): base, flip(19)                       -> 1 (last byte)
    #  run G (2): "", ""                               -> 0
    #  run H (1): solo
    #  run I (3): base, base + "!", base               -> 2 (length, twice)
    order = ([8, 0, 1, 2, 3, 4, 5, 6, 7] + [9, 10, 11] + [9, 12] + [10, 13] + [9, 14] + [10, 15]
             + [16, 17] + [19] + [9, 18, 10])
    keys = [1] * 9 + [2] * 3 + [3] * 2 + [4] * 2 + [5] * 2 + [6] * 2 + [7] * 2 + [8] + [9] * 3
    want = ref.verify_runs(keys, order, offsets, data.tobytes(), len(strings))
    assert want[1:] == (7, 0)
    assert [sum(1 for x in keys if x == r) for r in range(1, 10)] == [9, 3, 2, 2, 2, 2, 2, 1, 3]
    info0 = torch.tensor([1000, 50], dtype=torch.int64, device="cuda")
    head, info = _verify(ctx, keys, order, offsets, data, info=info0, k=5)
    assert head == want[0]
    assert info == [1007, 50]  # added to, not overwritten
    # invalid: an index past the column, and offsets past the data
    bad_off = offsets.copy()
    bad_off[-1] += 1  # string 19 ends past the data
    order = [0, 1, 20, 2, 19, 19, 3]
    keys = [1] * 7
    want = ref.verify_runs(keys, order, bad_off, data.tobytes(), len(strings))
    # 1-0 equal; 20: invalid; 2-20: invalid; 19-2, 19-19: invalid; 3-19: invalid
    assert want == ([1, 0, 0, 0, 0, 0, 0], 5, 5)
    head, info = _verify(ctx, keys, order, bad_off, data)
    assert head == want[0] and info == [5, 5]


@pytest.mark.gpu
def test_verify_runs_more_than_one_pass_of_the_grid(ctx, corpus):
    """600 000 arrivals: every string of the corpus many times, grouped by key;
    one copy is replaced by a different string."""
    offsets, data = corpus
    m = 600_000
    order = np.sort(np.random.default_rng(4).integers(0, N_STR, m)).astype(np.uint32)
    keys = order.astype(np.int64) * 1_000_003 - 17
    head, info = _verify(ctx, keys, order, offsets, data, k=1)
    assert info == [0, 0]
    assert np.array_equal(np.asarray(head), np.concatenate([[1], np.diff(order) != 0]))
    j = int(np.nonzero(order == 31)[0][5])
    order[j] = 32  # the 300-byte string: differs from its predecessor and from its successor
    head2, info = _verify(ctx, keys, order, offsets, data, k=1)
    assert info == [2, 0] and head2 == head


@pytest.mark.gpu
def test_nothing_and_bad_arguments(ctx, corpus):
    offsets, data = corpus
    lib, h = ctx.lib, ctx.handle
    off_t, dat_t = _dev(offsets), _dev(data)
    rec = _dev(np.array([1, 2], dtype=np.int64))
    out_off = _dev(np.array([0, 0, 0], dtype=np.int64))
    out_len = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    head = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
    keys = _dev(np.array([1, 1], dtype=np.int64))
    info = torch.tensor([3, 4], dtype=torch.int64, device="cuda")
    s, L, n = _sptr(), data.size, N_STR
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    # m == 0: a no-op, NULL per-element pointers allowed
    assert lib.dpg_string_lengths(h, None, L, n, None, 0, None, p(info), s) == OK
    assert lib.dpg_string_pack(h, None, p(dat_t), L, n, None, 0, None, p(out), 64, p(info),
                               s) == OK
    assert lib.dpg_string_verify_runs(h, None, None, None, p(dat_t), L, n, 0, None, p(info),
                                      s) == OK
    # NULL pointers
    assert lib.dpg_string_lengths(h, p(off_t), L, n, p(rec), 2, p(out_len), None,
                                  s) == INVALID_ARG
    assert lib.dpg_string_lengths(h, None, L, n, p(rec), 2, p(out_len), p(info),
                                  s) == INVALID_ARG
    assert lib.dpg_string_lengths(h, p(off_t), L, n, p(rec), 2, None, p(info), s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), None, L, n, p(rec), 2, p(out_off), p(out), 64,
                               p(info), s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, n, p(rec), 2, None, p(out), 64,
                               p(info), s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, n, p(rec), 2, p(out_off), None, 64,
                               p(info), s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, n, p(rec), 2, p(out_off), p(out), 64,
                               None, s) == INVALID_ARG
    assert lib.dpg_string_verify_runs(h, None, None, p(off_t), p(dat_t), L, n, 2, p(head),
                                      p(info), s) == INVALID_ARG
    assert lib.dpg_string_verify_runs(h, p(keys), None, p(off_t), p(dat_t), L, n, 2, None,
                                      p(info), s) == INVALID_ARG
    assert lib.dpg_string_verify_runs(h, p(keys), None, p(off_t), p(dat_t), L, n, 2, p(head),
                                      None, s) == INVALID_ARG
    # negative counts
    assert lib.dpg_string_lengths(h, p(off_t), L, n, p(rec), -1, p(out_len), p(info),
                                  s) == INVALID_ARG
    assert lib.dpg_string_lengths(h, p(off_t), -1, n, p(rec), 2, p(out_len), p(info),
                                  s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, -1, p(rec), 2, p(out_off), p(out), 64,
                               p(info), s) == INVALID_ARG
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, n, p(rec), 2, p(out_off), p(out), -1,
                               p(info), s) == INVALID_ARG
    assert lib.dpg_string_verify_runs(h, p(keys), None, p(off_t), p(dat_t), L, -1, 2, p(head),
                                      p(info), s) == INVALID_ARG
    assert lib.dpg_string_verify_runs(h, p(keys), None, p(off_t), p(dat_t), L, n, -2, p(head),
                                      p(info), s) == INVALID_ARG
    # counts of 2^31 and more
    assert lib.dpg_string_lengths(h, p(off_t), L, n, p(rec), 1 << 31, p(out_len), p(info),
                                  s) == UNSUPPORTED
    assert lib.dpg_string_pack(h, p(off_t), p(dat_t), L, 1 << 31, p(rec), 2, p(out_off), p(out),
                               64, p(info), s) == UNSUPPORTED
    assert lib.dpg_string_verify_runs(h, p(keys), None, p(off_t), p(dat_t), L, n, 1 << 31,
                                      p(head), p(info), s) == UNSUPPORTED
    torch.cuda.synchronize()
    # nothing on the device was touched
    assert info.tolist() == [3, 4]
    assert out_len.tolist() == [-7, -7] and head.tolist() == [9, 9]
    assert bool((out == 0xEE).all())
    from pipelinedp_amd import _native
    with pytest.raises(_native.NativeError, match="invalid argument"):
        ctx.string_pack(off_t.data_ptr(), dat_t.data_ptr(), L, n, rec.data_ptr(), 2,
                        out_off.data_ptr(), out.data_ptr(), 64, None, s)
