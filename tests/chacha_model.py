"""The model the random-scalar stream (csrc/chacha.h, csrc/random.hip, trh_rng_*) is tested against; no GPU, nothing of the library.

Element i of the stream (seed, stream id), as include/trh.h states it:
  1. ChaCha20 block number i -- RFC 8439 section 2.3's block function, 20 rounds, over the original 64 + 64 layout: state words 12 - 13 the 64-bit
     block counter (low word first), words 14 - 15 the 64-bit stream id;
  2. its 64 bytes as eight little-endian u64 limbs;
  3. (limbs[0 .. 4) + 2^256 limbs[4 .. 8)) mod m, stored as four u64 Montgomery words.
block() is written from the RFC, word by word in Python integers; blocks() is the same over a numpy vector of block numbers (what the GPU
tests compare 2^16 elements against); from_u512 uses Python integers and oracle/pasta.py's moduli.  tests/test_rng_host.py pins all of it
by RFC 8439's section 2.3.2 vector, the all-zero key's well-known first block, and that block's value in both fields."""
import numpy as np

import pasta as o

SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"
M32 = 0xFFFFFFFF


def key_words(seed: bytes):
    assert len(seed) == 32
    return [int.from_bytes(seed[4 * i:4 * i + 4], "little") for i in range(8)]


def _rotl(v, c):
    return ((v << c) & M32) | (v >> (32 - c))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


_ROUNDS = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def block(seed: bytes, counter: int, stream_id: int = 0) -> bytes:
    """the 64 bytes of block `counter`"""
    assert 0 <= counter < 1 << 64 and 0 <= stream_id < 1 << 64
    init = list(SIGMA) + key_words(seed) + [counter & M32, counter >> 32, stream_id & M32, stream_id >> 32]
    x = list(init)
    for _ in range(10):
        for q in _ROUNDS:
            _quarter(x, *q)
    return b"".join(((a + b) & M32).to_bytes(4, "little") for a, b in zip(x, init))


def blocks(seed: bytes, counters, stream_id: int = 0) -> np.ndarray:
    """block(seed, c, stream_id) for every c of `counters` (any integers below 2^64) as an (n, 16) array of u32 words"""
    c = np.array([int(v) for v in counters], dtype=np.uint64)
    n = len(c)
    init = [np.full(n, w, np.uint32) for w in list(SIGMA) + key_words(seed)]
    init += [(c & np.uint64(M32)).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32),
             np.full(n, stream_id & M32, np.uint32), np.full(n, stream_id >> 32, np.uint32)]
    x = [v.copy() for v in init]

    def rotl(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    with np.errstate(over="ignore"):
        for _ in range(10):
            for a, b, cc, d in _ROUNDS:
                x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 16)
                x[cc] = x[cc] + x[d]; x[b] = rotl(x[b] ^ x[cc], 12)
                x[a] = x[a] + x[b]; x[d] = rotl(x[d] ^ x[a], 8)
                x[cc] = x[cc] + x[d]; x[b] = rotl(x[b] ^ x[cc], 7)
        return np.stack([a + b for a, b in zip(x, init)], axis=1)


def from_u512(field: str, data: bytes) -> int:
    """64 bytes -> the canonical value of from_u512's result"""
    assert len(data) == 64
    return int.from_bytes(data, "little") % o.FIELDS[field].m


def element(field: str, seed: bytes, index: int, stream_id: int = 0) -> int:
    """canonical value of element `index`"""
    return from_u512(field, block(seed, index, stream_id))


def elements_limbs(field: str, seed: bytes, first: int, n: int, stream_id: int = 0) -> np.ndarray:
    """elements first .. first + n - 1 as (n, 4) u64 Montgomery words -- the memory image a fill leaves"""
    f = o.FIELDS[field]
    words = blocks(seed, [first + i for i in range(n)], stream_id)
    out = np.empty((n, 4), np.uint64)
    for i, row in enumerate(words):
        out[i] = f.limbs(int.from_bytes(row.astype("<u4").tobytes(), "little") % f.m)
    return out
