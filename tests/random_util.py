"""Reference for the random-element tests (tests/test_random.py): ChaCha20 as rand_chacha 0.3's ChaCha20Rng lays it out, vectorised over
blocks with numpy uint32 arrays, and Fr::from_bytes_wide / Fr::random of halo2curves 0.3.1 in Python integers, written from the
definitions alone -- nothing here calls the library.  What pins the block function is rand_chacha's zero-seed vector and RFC 7539 2.3.2.
    state = "expand 32-byte k" | key (8 words) | 64-bit block counter (words 12, 13) | 64-bit stream id (words 14, 15)
    element i of a stream = (block (first_block + i) read as one little-endian 512-bit integer) mod r, stored Montgomery (R = 2^256)
Arrays are numpy: blocks (n, 64) uint8, Fr (n, 4) uint64."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MONT = 1 << 256
RR = MONT % R
H2HIP_EINVAL = 1
SIGMA = (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)


def _rotl(x, s):
    return (x << np.uint32(s)) | (x >> np.uint32(32 - s))


def _quarter(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(seed, counters, stream_id=0):
    """blocks `counters` (integers below 2^64) of the stream keyed by the 32-byte seed -> (n, 64) uint8"""
    seed = bytes(seed)
    assert len(seed) == 32 and 0 <= stream_id < 1 << 64
    counters = [int(c) for c in counters]
    assert all(0 <= c < 1 << 64 for c in counters)
    n = len(counters)
    init = np.empty((16, n), dtype=np.uint32)
    for i in range(4):
        init[i] = SIGMA[i]
    for i, w in enumerate(np.frombuffer(seed, dtype="<u4")):
        init[4 + i] = w
    ctr = np.array(counters, dtype=np.uint64).reshape(n)
    init[12] = (ctr & np.uint64(0xffffffff)).astype(np.uint32)
    init[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    init[14] = stream_id & 0xffffffff
    init[15] = stream_id >> 32
    x = init.copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
            _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
        x += init
    return np.ascontiguousarray(x.T).astype("<u4").view(np.uint8).reshape(n, 64)


def limbs(values):
    """integers below 2^256 -> (n, 4) uint64"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def wide_ints(data):
    """(n, 64) uint8 -> n integers below 2^512"""
    return [int.from_bytes(bytes(row), "little") for row in np.asarray(data, dtype=np.uint8).reshape(-1, 64)]


def fr_from_bytes_wide(data):
    """Fr::from_bytes_wide over (n, 64) uint8 -> (n, 4) uint64 Montgomery"""
    return limbs([v % R * RR % R for v in wide_ints(data)])


def fr_random(seed, n, first_block=0, stream_id=0):
    """n consecutive draws of Fr::random from ChaCha20Rng::from_seed(seed) positioned at block first_block"""
    return fr_random_at(seed, range(first_block, first_block + n), stream_id)


def fr_random_at(seed, counters, stream_id=0):
    """the draws at the given block numbers (the generator is random-access)"""
    counters = list(counters)
    if not counters:
        return np.zeros((0, 4), dtype=np.uint64)
    return fr_from_bytes_wide(chacha20_blocks(seed, counters, stream_id))


def crafted_wide():
    """the edge strings of tests/cpp/test_random_host.cpp as (n, 64) uint8"""
    m = MONT - 1
    vals = [0, 1, R - 1, R, R + 1, m, MONT, R * MONT, (1 << 512) - 1, m, m << 256, (R - 1) << 256 | (R - 1), (R << 256) + R, 1 << 511]
    return np.frombuffer(b"".join(v.to_bytes(64, "little") for v in vals), dtype=np.uint8).reshape(-1, 64).copy()
