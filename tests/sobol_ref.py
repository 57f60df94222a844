"""numpy restatement of the Owen-scrambled Sobol sampler (include/fspt.h FSPT_SAMPLER_SOBOL).

Everything is uint32 arithmetic that wraps modulo 2^32.  `value` takes arrays (broadcast) and returns float32.
"""
import numpy as np

U32 = np.uint32


def _u(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32)


def rev(x):
    x = _u(x).copy()
    x = ((x >> U32(1)) & U32(0x55555555)) | ((x & U32(0x55555555)) << U32(1))
    x = ((x >> U32(2)) & U32(0x33333333)) | ((x & U32(0x33333333)) << U32(2))
    x = ((x >> U32(4)) & U32(0x0F0F0F0F)) | ((x & U32(0x0F0F0F0F)) << U32(4))
    x = ((x >> U32(8)) & U32(0x00FF00FF)) | ((x & U32(0x00FF00FF)) << U32(8))
    return (x >> U32(16)) | (x << U32(16))


def lk(x, s):
    x = (_u(x) + _u(s)).astype(np.uint32)
    for c in (0x6C50B47C, 0xB82F1E52, 0xC7AFE638, 0x8D22F6E6):
        x = x ^ (x * U32(c))
    return x


def nus(x, s):
    return rev(lk(rev(x), s))


def h(x):
    x = _u(x)
    x = x ^ (x >> U32(16))
    x = x * U32(0x7FEB352D)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846CA68B)
    return x ^ (x >> U32(16))


def sobol0(i):
    return rev(i)


def sobol1(i):
    """The issue's loop, vectorised: r ^= v for every set bit of i, v ^= v >> 1 per bit."""
    i = _u(i).copy()
    r = np.zeros_like(i)
    v = np.full_like(i, 1 << 31)
    for _ in range(32):
        r = np.where(i & U32(1), r ^ v, r)
        i = i >> U32(1)
        v = v ^ (v >> U32(1))
    return r


def value_bits(seed, pixel, sample, dim):
    """The scrambled 32-bit value before the float conversion."""
    seed, pixel, sample, dim = np.broadcast_arrays(_u(seed), _u(pixel), _u(sample), _u(dim))
    with np.errstate(over="ignore"):
        key = h(seed ^ h(pixel ^ h((dim >> U32(1)) + U32(0x9E3779B9))))
        i = nus(sample, key)
        x = np.where(dim & U32(1), sobol1(i), sobol0(i))
        return nus(x, h(key ^ (U32(0x68BC21EB) + (dim & U32(1)))))


def value(seed, pixel, sample, dim):
    x = value_bits(seed, pixel, sample, dim)
    return ((x >> U32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
