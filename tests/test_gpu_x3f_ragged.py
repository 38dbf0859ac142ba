"""gemm_x3f_ragged (mtrl_amd/csrc/gemm_x3f_impl.h, tag 16): the split2h ReLU-mask data grad of the actor
step over each critic member's active rows only, against the dense launch on the same inputs with the
inactive rows of A zeroed (so the plane exponents agree).  Every active output row must equal the dense
row rows_e[slot] bit for bit, the output record's exponent and the max over its partial maxima must be
equal, and nothing but the live rows may be written: the ragged outputs start as 0xFF bytes and the
record's partial maxima as 1e30, so a store past n_e or a stale slot of a workgroup that left early shows.

Shapes: E = 2, B = 640 rows per member (up to 4 row tiles of 208 each), N = 512 (two column tiles; 504: a
partial one), K = 128 (two main-loop steps); the debug entry point launches whatever the tile count."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, K = 640, 128
CASES = [(417, 223), (208, 432), (1, 639), (0, 640), (640, 640)]


def _active(n0, n1, rng):
    """[2][B] bytes: n0 / n1 active rows; every row is active in at least one member when n0 + n1 >= B"""
    act = np.zeros((2, B), np.uint8)
    perm = rng.permutation(B)
    act[0, perm[:n0]] = 1
    rest = perm[n0:]  # rows member 0 left out come first in member 1
    order = np.concatenate([rest, perm[:n0]])
    act[1, order[:n1]] = 1
    assert act[0].sum() == n0 and act[1].sum() == n1
    return act


def _run(n0, n1, N, planes):
    from mtrl_amd import _lib as L

    lib = L.load()
    rng = np.random.default_rng(1000 * n0 + n1 + N)
    A = (rng.standard_normal((2, B, K)) * 1e-3).astype(np.float32)
    W = (rng.standard_normal((2, N, K)) / np.sqrt(K)).astype(np.float32)
    mask = rng.standard_normal((2, B, N)).astype(np.float32)
    act = _active(n0, n1, rng)
    dt = np.uint16 if planes else np.float32
    shape = (2, 2, B, N) if planes else (2, B, N)
    dense, rag = np.zeros(shape, dt), np.zeros(shape, dt)
    rows = np.zeros((2, B), np.int32)
    info = np.zeros(6, np.int32)
    flags = (1 if planes else 0) | (2 if N % 16 == 0 else 0)
    L.check(lib.mtsac_debug_gemm_x3f_ragged(flags, B, N, K, A.ctypes.data, W.ctypes.data, mask.ctypes.data,
                                            act.ctypes.data, dense.ctypes.data, rag.ctypes.data, rows.ctypes.data,
                                            info.ctypes.data))
    return act, dense, rag, rows, info


@pytest.mark.parametrize("planes", [True, False], ids=["planes", "fp32"])
@pytest.mark.parametrize("n0,n1,N", [(a, b, 512) for a, b in CASES] + [(417, 223, 504)],
                         ids=[f"{a}_{b}" for a, b in CASES] + ["417_223_n504"])
def test_ragged_rows_equal_dense(n0, n1, N, planes):
    act, dense, rag, rows, info = _run(n0, n1, N, planes)
    assert (int(info[4]), int(info[5])) == (n0, n1)
    poison = np.uint16(0xFFFF) if planes else np.uint32(0xFFFFFFFF)
    ragb = rag if planes else rag.view(np.uint32)
    denb = dense if planes else dense.view(np.uint32)
    for e, n in enumerate((n0, n1)):
        want_rows = np.flatnonzero(act[e])  # ascending
        np.testing.assert_array_equal(rows[e, :n], want_rows)
        got = ragb[e][:, :n] if planes else ragb[e][:n]
        want = denb[e][:, want_rows] if planes else denb[e][want_rows]
        np.testing.assert_array_equal(got, want)
        tail = ragb[e][:, n:] if planes else ragb[e][n:]
        assert np.all(tail == poison), "a store past the member's live rows"
        # the dense rows of an inactive pair are zero: dropping them loses nothing
        off = np.flatnonzero(act[e] == 0)
        assert not np.any(denb[e][:, off] if planes else denb[e][off])
    assert np.any(denb != 0)
    if planes:  # the record: exponent written once, no stale partial maximum
        assert int(info[0]) == int(info[1])
        assert info[2:4].view(np.float32)[0] == info[2:4].view(np.float32)[1] > 0
