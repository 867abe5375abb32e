"""The ensemble's random generator (include/eqf_ensemble_random.h) restated in numpy: Philox4x64-10 on uint64 with the high word of a product formed from
32-bit halves, the word-to-uniform map U, the Box-Muller normals and the uniforms, laid out over counters exactly as the header states. Nothing here calls the
product; tests/test_ensemble_random_cases.py pins the restatement word for word to np.random.Philox, tests/test_gpu_ensemble_random.py holds the device to it.
Results are cached: a reference is computed once and shared by the tests that need it."""
import functools

import numpy as np

M0, M1 = np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157)
W0, W1 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B)
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MASK64 = (1 << 64) - 1


def u64(v):
    """a Python int taken modulo 2^64"""
    return np.uint64(int(v) & MASK64)


def mulhi(a, b):
    """the high 64 bits of a * b (uint64 arrays or scalars), from 32-bit halves"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    a0, a1, b0, b1 = a & MASK32, a >> S32, b & MASK32, b >> S32
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (ll >> S32) + (lh & MASK32) + (hl & MASK32)  # < 3 * 2^32
    return hh + (lh >> S32) + (hl >> S32) + (mid >> S32)


def philox4x64_10(seed, stream, c0, c1, c2, c3):
    """the four words of every counter (c0, c1, c2, c3) (arrays broadcast) under the key (seed, stream)"""
    with np.errstate(over="ignore"):
        c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)))
        k0, k1 = u64(seed), u64(stream)
        for _ in range(10):
            hi0, lo0, hi1, lo1 = mulhi(M0, c0), M0 * c0, mulhi(M1, c2), M1 * c2
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = k0 + W0, k1 + W1
    return c0, c1, c2, c3


def unit(x):
    """U(x) = (2 (x >> 12) + 1) 2^-53"""
    x = np.asarray(x, np.uint64)
    return ((x >> np.uint64(12)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0**-53


def normals(seed, stream, rows, P):
    """(rows, P): rows 4 j .. 4 j + 3 of particle k from counter (j, k, 0, 0); (x0, x1) and (x2, x3) are the Box-Muller pairs"""
    nb = (rows + 3) // 4
    j, k = np.meshgrid(np.arange(nb, dtype=np.uint64), np.arange(P, dtype=np.uint64), indexing="ij")
    x = philox4x64_10(seed, stream, j, k, np.uint64(0), np.uint64(0))
    out = np.zeros((4 * nb, P))
    for h in (0, 1):
        r = np.sqrt(-2.0 * np.log(unit(x[2 * h])))
        ang = 2.0 * np.pi * unit(x[2 * h + 1])
        out[2 * h::4] = r * np.cos(ang)
        out[2 * h + 1::4] = r * np.sin(ang)
    return np.asfortranarray(out[:rows])


def uniforms(seed, stream, count):
    """draw i = U(word i & 3 of counter (i >> 2, 0, 0, 1))"""
    nb = (count + 3) // 4
    x = philox4x64_10(seed, stream, np.arange(nb, dtype=np.uint64), np.uint64(0), np.uint64(0), np.uint64(1))
    return np.ascontiguousarray(unit(np.stack(x, axis=1).reshape(-1))[:count])


@functools.lru_cache(maxsize=None)
def cached_normals(seed, stream, rows, P):
    out = normals(seed, stream, rows, P)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cached_uniforms(seed, stream, count):
    out = uniforms(seed, stream, count)
    out.setflags(write=False)
    return out


def numpy_block(seed, stream, counter):
    """np.random.Philox's four raw words at `counter` (a 256-bit int, word 0 least significant): numpy increments before it generates, so it starts one below"""
    c = (counter - 1) % (1 << 256)
    words = [(c >> (64 * i)) & MASK64 for i in range(4)]
    bg = np.random.Philox(key=np.array([int(seed) & MASK64, int(stream) & MASK64], np.uint64), counter=np.array(words, np.uint64))
    return bg.random_raw(4)


def gaussian_summary(z):
    """(|mean| sqrt(n), |var - 1| / sqrt(2 / n), Kolmogorov distance sqrt(n)) of the flattened sample against N(0, 1)"""
    from math import erf, sqrt

    z = np.sort(np.asarray(z, float).reshape(-1))
    n = z.size
    cdf = 0.5 * (1.0 + np.array([erf(v / sqrt(2.0)) for v in z]))
    i = np.arange(1, n + 1)
    ks = max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    return abs(float(z.mean())) * sqrt(n), abs(float(z.var()) - 1.0) / sqrt(2.0 / n), ks * sqrt(n)
