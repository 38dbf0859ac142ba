"""Host model of the device noise stream (mtrl_amd/csrc/devrng.h): Philox4x32-10 from its published definition
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain Python integers, and
`uniform4` / `normal4` as devrng.h builds them on top of it.

 * counter words {row, stream, counter lo, counter hi}, key {seed lo, seed hi};
 * [0, 1): (x >> 8) 2^-24; (0, 1]: ((x >> 8) + 1) 2^-24 -- both exact in float32;
 * Box-Muller: r = sqrt(-2 ln u1), t = float32(2 pi) u2 rounded to float32 as the device rounds it, then
   r cos t, r sin t with log, sqrt, cos, sin evaluated in float64 AT those float32 arguments.  What separates
   the device's float32 result from this model is then the error of its logf, sqrtf, cosf / sinf and the two
   roundings of -2 ln u and of the product: `normal_bound`.

The policy heads draw `normal4(seed, stream_id + 16 (lane >> 2), counter, row)[lane & 3]` for action lane `lane`
(heads.hip policy_finish, heads_wide.h policy_finish_wide): `policy_eps`.
"""

from __future__ import annotations

import math

import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # golden ratio, sqrt(3) - 1
TWO_PI_F32 = np.float32(6.28318530717958647692)

# ulp errors of the device's float32 functions: the OpenCL full-profile limits (log 3, sin / cos 4), taken because
# the ROCm toolkit ships no accuracy table of its device library; sqrt is correctly rounded (one of the roundings).
ULPS_LOG, ULPS_TRIG = 3, 4


def philox4x32_10(ctr, key):
    """(c0, c1, c2, c3), (k0, k1) -> the four output words; ten rounds, the key bumped between rounds."""
    c0, c1, c2, c3 = (int(c) & M32 for c in ctr)
    k0, k1 = (int(k) & M32 for k in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
    return c0, c1, c2, c3


def words(seed, stream, counter, row):
    seed, counter = int(seed), int(counter)
    return philox4x32_10((int(row) & M32, int(stream) & M32, counter & M32, (counter >> 32) & M32),
                         (seed & M32, (seed >> 32) & M32))


def unit_halfopen(x: int) -> np.float32:  # [0, 1)
    return np.float32((x >> 8) * 2.0 ** -24)


def unit_open(x: int) -> np.float32:  # (0, 1]
    return np.float32(((x >> 8) + 1) * 2.0 ** -24)


def uniform4(seed, stream, counter, row) -> np.ndarray:
    return np.array([unit_halfopen(w) for w in words(seed, stream, counter, row)], np.float32)


def normal4_model(seed, stream, counter, row):
    """(values float64 [4], r [4]): the Box-Muller model and the radius of each value's pair."""
    w = words(seed, stream, counter, row)
    out, rad = [], []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        u = unit_open(a)
        t = float(np.float32(TWO_PI_F32 * unit_open(b)))  # one float32 product, as the device forms it
        r = math.sqrt(-2.0 * math.log(float(u)))
        out += [r * math.cos(t), r * math.sin(t)]
        rad += [r, r]
    return np.array(out, np.float64), np.array(rad, np.float64)


def normal4(seed, stream, counter, row) -> np.ndarray:
    return normal4_model(seed, stream, counter, row)[0]


def normal_bound(r):
    """The device's float32 normal against the model: (ulps_log + ulps_trig + 2) 2^-23 max(r, 1)."""
    return (ULPS_LOG + ULPS_TRIG + 2) * 2.0 ** -23 * np.maximum(np.asarray(r, np.float64), 1.0)


def policy_eps(seed, stream_id, counter, B, A, noise_div=0):
    """eps [B][A] the policy heads draw from the device stream, and each element's radius."""
    eps, rad = np.zeros((B, A)), np.zeros((B, A))
    for b in range(B):
        row = b // noise_div if noise_div > 0 else b
        for g in range((A + 3) // 4):
            v, r = normal4_model(seed, stream_id + 16 * g, counter, row)
            n = min(4, A - 4 * g)
            eps[b, 4 * g:4 * g + n], rad[b, 4 * g:4 * g + n] = v[:n], r[:n]
    return eps, rad


def stream_keys(streams, groups, counters, rows):
    """The Philox (stream word, counter, row) triples the heads use for these stream ids and lane groups."""
    return [(s + 16 * g, c, r) for s in streams for g in groups for c in counters for r in rows]
