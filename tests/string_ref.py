"""The 64-bit string key of include/dpg.h ("string columns"), restated from its
text with Python integers: length mix, word loop, reserved-key remap.  Slow on
purpose -- one string at a time, no numpy arithmetic that could share a bug
with pipelinedp_amd.string_columns.host_keys."""
import numpy as np

M64 = (1 << 64) - 1
KEYDICT_EMPTY = 1 << 63
LEN_MUL = 0x9E3779B97F4A7C15


def fmix64(k: int) -> int:
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    return k ^ (k >> 33)


def key(s: bytes, seed: int = 0) -> int:
    """The key of one string as an unsigned 64-bit integer."""
    h = fmix64((seed & M64) ^ ((len(s) * LEN_MUL) & M64))
    for k in range(0, len(s), 8):
        # int.from_bytes of a short last chunk: the missing high bytes are zero
        h = fmix64(h ^ int.from_bytes(s[k:k + 8], "little"))
    return KEYDICT_EMPTY ^ 1 if h == KEYDICT_EMPTY else h


def keys(strings, seed: int = 0) -> np.ndarray:
    """Keys of a sequence of bytes objects as int64 bit patterns."""
    return np.array([key(s, seed) for s in strings], dtype=np.uint64).view(np.int64)


def keys_of_column(offsets, data, seed: int = 0) -> np.ndarray:
    """Keys of the records of an (offsets, data) column with valid offsets."""
    buf = bytes(np.asarray(data, dtype=np.uint8))
    off = [int(x) for x in np.asarray(offsets)]
    return keys([buf[a:b] for a, b in zip(off[:-1], off[1:])], seed)
