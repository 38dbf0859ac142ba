"""tests/philox_ref.py against the published Philox4x32-10 known answers, the unit-interval maps and Box-Muller
model's own properties, and the distinctness of the noise streams the policy heads use."""

import math

import numpy as np
import pytest

import philox_ref as P

# Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    assert P.philox4x32_10(ctr, key) == want


def test_word_order_and_unit_maps():
    # counter words {row, stream, counter lo, counter hi}, key {seed lo, seed hi}
    assert P.words(0x299F31D0A4093822, 0x85A308D3, 0x0370734413198A2E, 0x243F6A88) == KAT[2][2]
    assert P.unit_halfopen(0) == 0.0 and P.unit_halfopen(0xFFFFFFFF) == np.float32(1 - 2.0 ** -24)
    assert P.unit_open(0) == np.float32(2.0 ** -24) and P.unit_open(0xFFFFFFFF) == 1.0
    assert P.unit_halfopen(0x000001FF) == np.float32(2.0 ** -24)  # the low 8 bits are dropped
    u = P.uniform4(5, 3, 9, 1)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    assert np.array_equal(u, np.array([(w >> 8) * 2.0 ** -24 for w in P.words(5, 3, 9, 1)], np.float32))


def test_normal_model():
    v, r = P.normal4_model(1234, 2, 2**32 + 5, 7)
    w = P.words(1234, 2, 2**32 + 5, 7)
    u1, t1 = ((w[0] >> 8) + 1) * 2.0 ** -24, float(np.float32(np.float32(2 * math.pi) * np.float32(((w[1] >> 8) + 1) * 2.0 ** -24)))
    assert r[0] == r[1] == math.sqrt(-2 * math.log(u1))
    assert v[0] == r[0] * math.cos(t1) and v[1] == r[0] * math.sin(t1)
    # pairs lie on their circle, and the stream is standard normal to sampling accuracy
    assert abs(math.hypot(v[2], v[3]) - r[2]) < 1e-12
    x = np.concatenate([P.normal4(9, 1, c, row) for c in range(50) for row in range(50)])
    assert abs(x.mean()) < 4 / math.sqrt(len(x)) and abs(x.var() - 1) < 4 * math.sqrt(2 / len(x))
    assert P.normal_bound(0.5) == 9 * 2.0 ** -23 and P.normal_bound(3.0) == 27 * 2.0 ** -23


def test_policy_eps_layout_and_shared_rows():
    eps, _ = P.policy_eps(11, 3, 5, 7, 19)
    for b in (0, 6):
        for j in (0, 3, 4, 18):
            assert eps[b, j] == P.normal4(11, 3 + 16 * (j >> 2), 5, b)[j & 3]
    shared, _ = P.policy_eps(11, 5, 5, 7, 4, noise_div=3)
    assert np.array_equal(shared[0], shared[2]) and np.array_equal(shared[3], shared[5])
    assert not np.array_equal(shared[2], shared[3])
    assert np.array_equal(shared[6], P.policy_eps(11, 5, 5, 3, 4)[0][2])


def test_streams_in_use_are_distinct():
    """Stream ids 1 .. 8 with the lane-group offsets 16 g, g = 0 .. 15 (A <= 64): no two (stream, group) pairs
    share a Philox stream word, so no two (stream word, counter, row) keys coincide; and the words differ."""
    keys = P.stream_keys(range(1, 9), range(16), (0, 1, 2**32 + 5), range(3))
    assert len(set(keys)) == len(keys) == 8 * 16 * 3 * 3
    sw = {s + 16 * g for s in range(1, 9) for g in range(16)}
    assert len(sw) == 8 * 16 and max(sw) == 8 + 240
    outs = {P.words(77, s, c, r) for s, c, r in keys}
    assert len(outs) == len(keys)
