"""
Philox4x32-10 restated in numpy for the sampler tests: the generator on a full four-word counter and two-word key (held
to the published known-answer vectors by tests/test_philox.py), the (seed, 64-bit counter, stream) form csrc/common.hpp
gives it, and that header's two maps of a 32-bit word to a uniform.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10_words(counter, key):
    """counter: four words, key: two words (each an int or an array of equal shape) -> the four 32-bit output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(*counter))
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def philox4x32_10(seed, counters, stream):
    """Philox4x32-10 as csrc/common.hpp forms it, for an array of 64-bit counters -> its four 32-bit words (x, y, z, w):
    key = the seed's low and high word, counter = (the counter's low word, its high word, stream, 0).  Counters wrap
    modulo 2^64 as the device's unsigned arithmetic does."""
    counters = np.asarray(counters, dtype=np.uint64)
    seed = int(seed)
    return philox4x32_10_words((counters & _M32, counters >> _S32, np.full_like(counters, stream), np.zeros_like(counters)),
                               (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def counters_u64(offset, index):
    """offset + index modulo 2^64 (python ints: numpy's uint64 addition would warn on the wrap)."""
    index = np.asarray(index)
    flat = [(int(offset) + int(i)) & 0xFFFFFFFFFFFFFFFF for i in index.reshape(-1)]
    return np.array(flat, dtype=np.uint64).reshape(index.shape)


def u32_to_unit(u):
    """[0, 1): (u >> 8) / 2^24, exact in float32 and float64."""
    return (np.asarray(u, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) / 16777216.0


def u32_to_unit_open0(u):
    """(0, 1]: ((u >> 8) + 1) / 2^24, exact in float32 and float64."""
    return ((np.asarray(u, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
