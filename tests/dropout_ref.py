"""NumPy model of the seeded dropout of the transformer heads (csrc/hp_philox.h, csrc/dropout_kernels.hip).

Philox4x32-10 over the flat row-major index space of a tensor: element e takes output word e & 3 of the block with counter
(lo32(e >> 2), hi32(e >> 2), lo32(stream), hi32(stream)) and key (lo32(seed), hi32(seed)); it is kept iff word >= T,
T = floor(p * 2^32 + 0.5); kept values are multiplied by float32(1 / (1 - p)) (0 when p = 1)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)      # both factors < 2^32: the product fits a uint64
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    assert 0.0 <= p <= 1.0
    return int(np.floor(float(p) * 4294967296.0 + 0.5))


def scale(p):
    return np.float32(0.0) if p >= 1.0 else np.float32(1.0 / (1.0 - float(p)))


def stream_id(step, site):
    return ((int(step) << 20) | int(site)) & MASK64


def random_words(n, first, seed, stream):
    """The uint32 word of elements first .. first + n - 1."""
    seed, stream = int(seed) & MASK64, int(stream) & MASK64
    first = int(first)
    b0, b1 = first >> 2, (first + n - 1) >> 2
    blk = np.arange(b0, b1 + 1, dtype=np.uint64)   # the blocks the elements touch, each computed once
    ones = np.ones_like(blk)
    out = philox4x32_10((blk & np.uint64(MASK32), blk >> np.uint64(32), ones * np.uint64(stream & MASK32), ones * np.uint64(stream >> 32)),
                        (seed & MASK32, seed >> 32))
    words = np.stack(out, axis=1).reshape(-1)      # word w of block b at 4 (b - b0) + w
    lead = first & 3
    return words[lead:lead + n]


def keep_mask(n, first, p, seed, stream):
    """bool (n,): True = kept."""
    if n == 0:
        return np.zeros(0, dtype=bool)
    return random_words(n, first, seed, stream).astype(np.uint64) >= np.uint64(threshold(p))


def dropout(x, addend, first, p, seed, stream):
    """float32: (kept ? x * scale : 0) [+ addend], the product and the sum each rounded once."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    keep = keep_mask(x.size, first, p, seed, stream).reshape(x.shape)
    y = np.where(keep, (x * scale(p)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    if addend is not None:
        y = (y + np.asarray(addend, dtype=np.float32)).astype(np.float32)
    return y
