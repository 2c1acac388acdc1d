"""The per-row draws of csrc/draw.hip restated in NumPy from the chain in include/ssdr_al.h: uint64 arithmetic masked to 32 bits, and
np.argsort(kind="stable") for the permutations.  Nothing here calls the library."""
import numpy as np

PERM, DUP, AUG_NOISE = 0, 1, 2
M32 = np.uint64(0xffffffff)
LANES = (0x9e3779b9, 0x85ebca6b)


def _u(x):
    return np.asarray(x, np.uint64)


def mix32(x):
    x = _u(x) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def state(c, seed, epoch, step, kind):
    seed = int(seed) & 0xffffffffffffffff
    s = mix32((seed & 0xffffffff) ^ c)
    s = mix32(s ^ np.uint64(seed >> 32))
    s = mix32(s ^ np.uint64(int(epoch) & 0xffffffff))
    s = mix32(s ^ np.uint64(int(step) & 0xffffffff))
    return mix32(s ^ np.uint64(int(kind) & 0xffffffff))


def word(seed, epoch, step, kind, e, j):
    """e: uint64 array of element indices, j: the word index"""
    e = _u(e)
    lo, hi = e & M32, e >> np.uint64(32)
    total = np.zeros(e.shape, np.uint64)
    for c in LANES:
        a = mix32(state(c, seed, epoch, step, kind) ^ lo)
        a = mix32((a + hi) & M32)
        a = mix32(a ^ np.uint64(j))
        total = (total + a) & M32
    return mix32(total)


def bits53(seed, epoch, step, kind, e, j):
    return (word(seed, epoch, step, kind, e, j) >> np.uint64(5)) * np.uint64(1 << 26) + (word(seed, epoch, step, kind, e, j + 1) >> np.uint64(6))


def perm_keys(seed, epoch, step, first_tile, num_tiles, num_points, key_bits=32):
    """uint64 [num_tiles, num_points]: the sort keys"""
    tile = (np.uint64(first_tile) + np.arange(num_tiles, dtype=np.uint64))[:, None]
    r = np.arange(num_points, dtype=np.uint64)[None, :]
    return word(seed, epoch, step, PERM, tile * np.uint64(1 << 32) + r, 0) >> np.uint64(32 - key_bits)


def perm(seed, epoch, step, num_tiles, num_points, first_tile=0, key_bits=32):
    keys = perm_keys(seed, epoch, step, first_tile, num_tiles, num_points, key_bits)
    return np.argsort(keys, axis=1, kind="stable").astype(np.int32)


def uniform(seed, epoch, step, kind, n, first=0):
    e = np.uint64(first) + np.arange(n, dtype=np.uint64)
    return ((word(seed, epoch, step, kind, e, 0) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def normal(seed, epoch, step, kind, n, scale=1.0, first=0):
    e = np.uint64(first) + np.arange(n, dtype=np.uint64)
    u1 = (bits53(seed, epoch, step, kind, e, 0) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = bits53(seed, epoch, step, kind, e, 2).astype(np.float64) * 2.0 ** -53
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    return np.float64(scale) * z
