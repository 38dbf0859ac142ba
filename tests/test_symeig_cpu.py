"""The float64 statement of the device eigenvalue solve (tests/symeig_ref.py) against numpy.linalg.eigvalsh and
the closed forms, the bar C_EIG it yields, and that the bar rejects planted faults.  No GPU."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import symeig_ref as S


@functools.lru_cache(maxsize=None)
def _cases():
    """[(name, A, closed form or None, eigvalsh)] computed once."""
    return [(name, A, cf, np.linalg.eigvalsh(A)) for name, A, cf in S.cpu_cases()]


def _worst(**faults):
    """Worst ratio over the cases, against eigvalsh and, where there is one, the closed form."""
    worst, where = 0.0, None
    for name, A, cf, ref in _cases():
        lam = S.sym_eigvals(A, **faults)[0]
        for want in (ref, cf):
            if want is None:
                continue
            q = S.ratio(lam, want)
            if q > worst:
                worst, where = q, name
    return worst, where


def test_statement_within_a_quarter_of_the_bar():
    worst, where = _worst()
    print(f"host statement: worst err / (r 2^-52 max|ref|) = {worst:.3g} at {where}; C_EIG = {S.C_EIG}")
    assert worst <= S.C_EIG / 4, (worst, where)
    # C_EIG is four times the measured worst ratio rounded up to a power of two, not more
    assert S.C_EIG == 2.0 ** np.ceil(np.log2(4 * worst))


def test_closed_forms_agree_with_eigvalsh():
    """The references themselves: eigvalsh stays within the same quarter bar of every closed form."""
    for name, A, cf, ref in _cases():
        if cf is not None:
            assert S.ratio(ref, cf) <= S.C_EIG / 4, name


def test_ascending_and_flags():
    for name, A, cf, ref in _cases():
        lam, flag, d, e = S.sym_eigvals(A)
        assert flag == 0 and np.all(np.diff(lam) >= 0), name


def test_tridiagonal_form_keeps_the_spectrum():
    for name, A, cf, ref in _cases():
        r = A.shape[0]
        d, e = S.tridiag(A)
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        assert S.ratio(np.linalg.eigvalsh(T), ref) <= S.C_EIG / 4, name


@pytest.mark.parametrize("fault", [dict(drop_last_step=True), dict(full_tau=True), dict(count_offset=1),
                                   dict(count_offset=-1), dict(halvings=20)],
                         ids=["dropped_last_step", "tau_for_half_tau", "sturm_plus_one", "sturm_minus_one", "20_halvings"])
def test_bar_rejects_planted_faults(fault):
    """A bar that lets one of these through is too loose: each must exceed the full C_EIG, not just C_EIG / 4."""
    worst, where = _worst(**fault)
    assert worst > S.C_EIG, (fault, worst, where)


def test_zero_matrix_exact_and_srank_one():
    from mtrl_amd import netmetrics as NM

    for r in (1, 2, 7, 33):
        lam, flag, d, e = S.sym_eigvals(np.zeros((r, r)))
        assert flag == 0 and lam.tobytes() == np.zeros(r).tobytes()
        assert NM.srank_from_singular_values(NM.singular_values_from_eigvals(lam)) == 1


def test_non_finite_entry_gives_nan_and_flag():
    A = S.gram_full(9, 3)
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[4, 2] = B[2, 4] = bad
        lam, flag, d, e = S.sym_eigvals(B)
        assert flag != 0 and np.all(np.isnan(lam))


def test_srank_from_eigvals_matches_srank_from_gram():
    """The device path's arithmetic: sqrt(max(lam, 0)) reversed through srank_from_singular_values."""
    from mtrl_amd import netmetrics as NM

    for seed in range(4):
        G = S.gram_full(24, seed)
        lam = np.linalg.eigvalsh(G)
        sig = NM.singular_values_from_eigvals(lam)
        assert sig.tobytes() == NM.singular_values_from_gram(G).tobytes()
        assert NM.srank_from_singular_values(sig) == NM.srank_from_gram(G)


class _DeviceEngine:
    """Stands in for MTSACEngine.network_metrics(eig="device"): eigenvalues instead of Grams."""

    def __init__(self, flags=0):
        self.flags, self.calls = flags, []

    def network_metrics(self, observations, eps, dormant, gram, threshold, eig="host"):
        self.calls.append((dormant, gram, eig))
        out = {}
        for name, E in (("actor", 1), ("critic", 2)):
            G = [[S.gram_full(12, 5 * e + i) for i in range(2)] for e in range(E)]
            out[name] = {"members": E, "depth": 2, "width": 12,
                         "counts": np.zeros((E, 2), np.int32) if dormant else None, "scores": None, "gram": None,
                         "eigvals": np.array([[np.linalg.eigvalsh(g) for g in m] for m in G]),
                         "eig_flags": np.full((E, 2), self.flags, np.int32), "_gram": G}
        return out


def test_compute_metrics_device_path():
    from mtrl_amd import netmetrics as NM
    from mtrl_amd.compat.config.utils import Metrics

    eng = _DeviceEngine()
    logs = NM.compute_metrics(eng, Metrics.ALL, None, None, eig="device")
    assert eng.calls == [(True, True, "device")]
    assert list(logs) == NM.expected_keys(2, 2, 2)
    ref = eng.network_metrics(None, None, True, True, 0.1)
    for name, e in (("actor", 0), ("critic_0", 0), ("critic_1", 1)):
        for i in range(2):
            want = NM.srank_from_gram(ref["actor" if name == "actor" else "critic"]["_gram"][e][i])
            assert logs[f"metrics/srank_{name}_torso_layer_{i}"] == want
    with pytest.raises(FloatingPointError):
        NM.compute_metrics(_DeviceEngine(flags=1), Metrics.SRANK, None, None, eig="device")
    with pytest.raises(ValueError):
        NM.compute_metrics(_DeviceEngine(), Metrics.ALL, None, None, eig="gpu")
