"""The symmetric eigenvalue kernels alone (mtsac_debug_sym_eigvals: sym_tridiag + tridiag_eigvals,
mtrl_amd/csrc/symeig.hip) at edge orders, against numpy.linalg.eigvalsh and the closed forms with the bar C_EIG
of tests/symeig_ref.py.  The debug entry keeps every device buffer between guard bands and follows the last
matrix with NaN words, so a store or a read outside the matrices fails the call or poisons the result."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import symeig_ref as S

pytestmark = pytest.mark.gpu


def _lib():
    from mtrl_amd import _lib as L

    return L, L.load()


def solve(As):
    """(lam [Z][r], d [Z][r], e [Z][r-1], flags [Z]) of the matrices As [Z][r][r]."""
    L, lib = _lib()
    A = np.ascontiguousarray(As, np.float64)
    Z, r, _ = A.shape
    keep = A.copy() if A.size < 1 << 20 else None
    lam, d, e = np.full((Z, r), -7.0), np.full((Z, r), -7.0), np.full((Z, r - 1), -7.0)
    flags = np.full(Z, -1, np.int32)
    L.check(lib.mtsac_debug_sym_eigvals(Z, r, A.ctypes.data, lam.ctypes.data, d.ctypes.data,
                                        e.ctypes.data if r > 1 else None, flags.ctypes.data))
    assert keep is None or np.array_equal(A, keep, equal_nan=True)  # the caller's matrices are read only
    return lam, d, e, flags


@functools.lru_cache(maxsize=None)
def _by_order():
    """{r: [(name, A, closed form or None, eigvalsh)]}: every case matrix and its references, computed once."""
    out = {}
    for name, A, cf in S.cases(S.GPU_SIZES):
        out.setdefault(A.shape[0], []).append((name, A, cf, np.linalg.eigvalsh(A)))
    return out


@functools.lru_cache(maxsize=None)
def _alone(r):
    """The single-matrix (Z = 1) results of every case of order r."""
    return [solve(A[None]) for _, A, _, _ in _by_order()[r]]


ORDERS = sorted(set(S.GPU_SIZES) | {21})


def test_orders_cover_the_cases():
    assert sorted(_by_order()) == ORDERS


@pytest.mark.parametrize("r", ORDERS)
def test_bar_against_eigvalsh_and_closed_forms(r):
    worst = 0.0
    for (name, A, cf, ref), (lam, d, e, flags) in zip(_by_order()[r], _alone(r)):
        lam, d, e = lam[0], d[0], e[0]
        assert flags[0] == 0, name
        assert np.all(np.isfinite(lam)) and np.all(np.diff(lam) >= 0), name
        for want in (ref, cf):
            if want is not None:
                q = S.ratio(lam, want)
                worst = max(worst, q)
                assert np.max(np.abs(lam - np.sort(want))) <= S.bar(r, want), (name, q)
        # the reduction alone: the returned tridiagonal matrix has the spectrum
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        q = S.ratio(np.linalg.eigvalsh(T), ref)
        worst = max(worst, q)
        assert np.max(np.abs(np.linalg.eigvalsh(T) - ref)) <= S.bar(r, ref), (name, "tridiagonal form", q)
        if name.startswith("zero"):
            assert lam.tobytes() == np.zeros(r).tobytes() and not d.any() and not e.any()
    print(f"r = {r}: worst err / (r 2^-52 max|ref|) = {worst:.3g} of C_EIG = {S.C_EIG}")


def test_largest_order():
    """r = 8192, the largest order (128 KiB of LDS in the bisection, offsets past 2^29 bytes in the matrix).  The
    (2, -1) Toeplitz matrix is tridiagonal already, so every column step takes the tau = 0 path and the
    reduction must return its diagonals untouched; the spectrum has a closed form."""
    r = 8192
    i = np.arange(r)
    A = np.zeros((1, r, r))
    A[0, i, i], A[0, i[:-1], i[1:]], A[0, i[1:], i[:-1]] = 2.0, -1.0, -1.0
    want = np.sort(2.0 - 2.0 * np.cos(np.arange(1, r + 1) * np.pi / (r + 1)))
    lam, d, e, flags = solve(A)
    assert flags[0] == 0 and np.all(d[0] == 2.0) and np.all(e[0] == -1.0)
    assert np.all(np.diff(lam[0]) >= 0)
    q = S.ratio(lam[0], want)
    print(f"r = {r}: err / (r 2^-52 max|ref|) = {q:.3g} of C_EIG = {S.C_EIG}")
    assert np.max(np.abs(lam[0] - want)) <= S.bar(r, want)


def test_trivial_orders_are_copies():
    """r = 1: d_0 = a_00; r = 2: d = the diagonal, e_0 = a_10; no arithmetic in the reduction."""
    for r in (1, 2):
        for (name, A, _, _), (lam, d, e, flags) in zip(_by_order()[r], _alone(r)):
            assert d[0].tobytes() == np.diag(A).copy().tobytes(), name
            if r == 2:
                assert e[0, 0] == A[1, 0], name


@pytest.mark.parametrize("r", ORDERS)
def test_bitwise_repeatable_and_independent_of_the_batch(r):
    cases, alone = _by_order()[r], _alone(r)
    n = len(cases)
    for g in range(0, n, 3):  # every case sits in one batch of 3 (the last batch repeats the last case)
        idx = [min(g + z, n - 1) for z in range(3)]
        batch = np.stack([cases[i][1] for i in idx])
        one, two = solve(batch), solve(batch)
        for a, b in zip(one, two):
            assert a.tobytes() == b.tobytes(), (cases[g][0], "two runs differ")
        for z, i in enumerate(idx):
            for a, b in zip(one, alone[i]):
                assert a[z].tobytes() == b[0].tobytes(), (cases[i][0], "alone and in a batch of 3 differ")


@pytest.mark.parametrize("r", [5, 65, 130])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_matrix_is_flagged_and_isolated(r, bad):
    """One non-finite entry (and its mirror): that matrix's row is all NaN with a set flag, and its two
    neighbours are bitwise what they are alone.  The kernels' trip counts do not depend on the data."""
    cases = _by_order()[r]
    batch = np.stack([cases[0][1], cases[0][1], cases[1][1]]).copy()
    i, j = r - 1, r // 2
    batch[1, i, j] = batch[1, j, i] = bad
    lam, d, e, flags = solve(batch)
    assert np.all(np.isnan(lam[1])) and flags[1] != 0
    assert flags[0] == 0 and flags[2] == 0
    for z, k in ((0, 0), (2, 1)):
        for a, b in zip((lam, d, e), _alone(r)[k]):
            assert a[z].tobytes() == b[0].tobytes()


def test_bad_arguments():
    L, lib = _lib()
    A, lam, fl = np.zeros((1, 2, 2)), np.zeros((1, 2)), np.zeros(1, np.int32)
    ok = (1, 2, A.ctypes.data, lam.ctypes.data, None, None, fl.ctypes.data)
    assert lib.mtsac_debug_sym_eigvals(*ok) == 0
    for k, v in ((0, 0), (0, -1), (1, 0), (1, -3), (2, None), (3, None), (6, None)):
        args = list(ok)
        args[k] = v
        assert lib.mtsac_debug_sym_eigvals(*args) == -22, (k, v)
