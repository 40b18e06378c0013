"""
CPU: the numpy Philox4x32-10 that the sampler tests restate the device's draws with (tests/helpers/philox.py), held to the
three published known-answer vectors of Philox4x32-10 (Random123's kat_vectors), and its (seed, counter, stream) wrapper
to the counter and key layout of csrc/common.hpp.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import philox  # noqa: E402

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_reproduces_the_published_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = tuple(int(w) for w in philox.philox4x32_10_words(counter, key))
        assert got == want, (counter, key, [hex(w) for w in got])
    # the same three as one array call
    counter = [np.array([c[i] for c, _, _ in KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[i] for _, k, _ in KNOWN_ANSWERS], dtype=np.uint64) for i in range(2)]
    got = np.stack(philox.philox4x32_10_words(counter, key), 1)
    assert got.tolist() == [list(w) for _, _, w in KNOWN_ANSWERS]


def test_wrapper_forms_counter_and_key_as_the_device_header_does():
    """key = (seed low, seed high); counter = (counter low, counter high, stream, 0)."""
    got = tuple(int(w) for w in philox.philox4x32_10(0x299f31d0a4093822, np.uint64(0x85a308d3243f6a88), 0x13198a2e))
    want = tuple(int(w) for w in philox.philox4x32_10_words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0)))
    assert got == want
    assert tuple(int(w) for w in philox.philox4x32_10(0, np.uint64(0), 0)) == KNOWN_ANSWERS[0][2]
    # an array of counters is the element-wise call, and the low word's wrap carries into the high word
    ctr = philox.counters_u64(2 ** 32 - 2, np.arange(4))
    assert [int(c) for c in ctr] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    words = philox.philox4x32_10(5, ctr, 0)
    for i, c in enumerate(ctr):
        c = int(c)
        assert tuple(int(w[i]) for w in words) == tuple(int(w) for w in philox.philox4x32_10_words((c & 0xffffffff, c >> 32, 0, 0), (5, 0)))
    assert int(philox.counters_u64(2 ** 64 - 1, np.array([2]))[0]) == 1


def test_uniform_maps():
    u = np.array([0, 255, 256, 0xffffffff], dtype=np.uint64)
    assert philox.u32_to_unit(u).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert philox.u32_to_unit_open0(u).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    for f in (philox.u32_to_unit, philox.u32_to_unit_open0):
        assert np.array_equal(f(u), f(u).astype(np.float32).astype(np.float64))
