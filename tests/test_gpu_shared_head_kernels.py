"""The head kernels with ONE head shared by all tasks (HeadParams::shared; MTSAC_NET_SHARED_HEAD), one by one.

 * The new weight and bias grad (head_backward_weight_shared: row chunks of R rows, per-chunk partials, a finish
   pass adding the chunks in ascending order) element by element against float64,
       dWh[e][w][o] = sum_b h[e][b][w] dout[e][b][o],   dbh[e][o] = sum_b dout[e][b][o]   over ALL B rows,
   under the project's own rule R.sum_bound(R.c_dot(B), sum |h dout|) (tests/sac_head_ref.py; no new constant),
   at hd in {1, 2, 8, 12}, E in {1, 3}, W in {4, 6, 260, 516} (W = 6: the scalar path; hd = 12, the wide family,
   only at W % 4 == 0) and B in {1, R - 1, R, R + 1, 2 R + 3}; two runs agree bitwise; the self-check word stays 0.
   Measured on one MI355X (R = 64): worst error / bound 0.66 for dWh (hd = 12, E = 3, W = 516, B = 63: one 63-link
   MFMA chain against c_dot(63) = 8), 0.18 for dbh; every case prints its own figure.
 * The forward (policy heads in every form, critic head in every mode) and the data grad with a shared head are the
   SAME kernel instances the multi-head path runs, so they are held bitwise to the multi-head kernels given T
   tied heads -- with the blocks of the tasks t > 0 poisoned (NaN) on the shared side: a kernel that still
   indexed the head by the row's task would return NaN.
"""

from __future__ import annotations

import contextlib

import numpy as np
import pytest

import sac_head_cases as C
import sac_head_ref as R
import test_gpu_head_kernels as HK

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
_p, _in, _nan, _same, _check, _lib = HK._p, HK._in, HK._nan, HK._same, HK._check, HK._lib
T_L = 3
WIDTHS = (4, 6, 260, 516)


@contextlib.contextmanager
def _shared():
    old = _lib().mtsac_debug_head_shared(1)
    try:
        yield
    finally:
        _lib().mtsac_debug_head_shared(old)


def run_shared_backward(B, E, W, hd, task, h, Wh, dout):
    o = dict(dz=_nan(E, B, W), db=_nan(E, W), dWh=_nan(E, W, hd), dbh=_nan(E, hd))
    info = np.zeros(8, np.int32)
    _check(_lib().mtsac_debug_head_backward_shared(B, T_L, E, W, hd, _p(task), _p(h), _p(Wh), _p(dout), _p(o["dz"]),
                                                   _p(o["db"]), _p(o["dWh"]), _p(o["dbh"]), _p(info)))
    o.update(data=int(info[0]), wgrad=int(info[1]), fault=int(info[2]), R=int(info[3]), chunks=int(info[4]))
    return o


def _case(hd, E, W, B, seed=0):
    rng = np.random.default_rng(7000 * hd + 100 * E + W + 7 * B + seed)
    h = np.maximum(rng.standard_normal((E, B, W)), 0).astype(f32)
    h.reshape(-1)[5::17] = -0.0
    Wh = (rng.standard_normal((E, W, hd)) / np.sqrt(W)).astype(f32)
    dout = rng.standard_normal((E, B, hd)).astype(f32)
    dout[rng.uniform(size=(E, B)) < 0.3] = 0.0
    task = (np.arange(B) % T_L).astype(np.int32)
    return h, Wh, dout, task


def _row_chunk():
    h, Wh, dout, task = _case(1, 1, 4, 1)
    return run_shared_backward(1, 1, 4, 1, task, h, Wh, dout)["R"]


@pytest.mark.parametrize("hd", [1, 2, 8, 12])
def test_shared_weight_grad(hd):
    Rc = _row_chunk()
    assert Rc >= 2
    worst = {"dWh": 0.0, "dbh": 0.0}
    for E in (1, 3):
        for W in WIDTHS:
            if hd > 8 and W % 4:
                continue  # the wide family runs at W % 4 == 0 only (head_kernels_cover)
            for B in (1, Rc - 1, Rc, Rc + 1, 2 * Rc + 3):
                h, Wh, dout, task = _case(hd, E, W, B)
                got = run_shared_backward(B, E, W, hd, task, h, Wh, dout)
                assert got["wgrad"] == 1 and got["fault"] == 0, (hd, E, W, B, got["fault"])
                assert got["chunks"] == -(-B // Rc)
                prod = h.astype(f64)[:, :, :, None] * dout.astype(f64)[:, :, None, :]  # [E][B][W][hd]
                want = dict(dWh=prod.sum(1), dbh=dout.astype(f64).sum(1))
                S = dict(dWh=np.abs(prod).sum(1), dbh=np.abs(dout.astype(f64)).sum(1))
                for k in ("dWh", "dbh"):
                    bound = R.sum_bound(R.c_dot(B), S[k])
                    print(f"hd={hd} E={E} W={W} B={B} {k}: worst err / bound {R.worst(got[k], want[k], bound):.3f}")
                    assert R.within(got[k], want[k], bound), (hd, E, W, B, k, R.worst(got[k], want[k], bound))
                    worst[k] = max(worst[k], R.worst(got[k], want[k], bound))
                again = run_shared_backward(B, E, W, hd, task, h, Wh, dout)
                for k in ("dWh", "dbh", "dz", "db"):
                    assert _same(got[k], again[k]), (hd, E, W, B, k, "two runs differ bitwise")
                # the data grad beside it: the multi-head kernels on T tied heads, bitwise
                tied = np.ascontiguousarray(np.repeat(Wh[:, None], T_L, axis=1))
                c = dict(hd=hd, E=E, W=W, T_l=T_L, B=B, task=task, h=h, Wh=tied, dout=dout)
                mh = HK.run_backward(c, 0)
                assert got["data"] == mh["ran"] == (1 if W % 4 == 0 else 0)
                for k in ("dz", "db"):
                    if W % 4:
                        assert np.isnan(got[k]).all()
                    else:
                        assert _same(got[k], mh[k]), (hd, E, W, B, k, "shared data grad differs from T tied heads")
    print(f"shared weight grad hd={hd}: row chunk {Rc}, worst err / bound {worst}")


def _poison(a, axis):
    """Blocks t > 0 of the task axis NaN: only block 0 may be read."""
    b = np.array(a, copy=True)
    idx = [slice(None)] * b.ndim
    idx[axis] = slice(1, None)
    b[tuple(idx)] = np.nan
    return b


@pytest.mark.parametrize("A", [1, 4, 6])
def test_shared_policy_forward_is_the_tied_multi_head_forward(A):
    for W in (4, 6, 260) if A <= 4 else (4, 260):
        base = C.policy_case(A, W, (5, 17, 3))
        tied = dict(base)
        tied["Wh"] = np.ascontiguousarray(np.repeat(base["Wh"][:1], base["T_l"], axis=0))
        tied["bh"] = np.ascontiguousarray(np.repeat(base["bh"][:1], base["T_l"], axis=0))
        shared = dict(tied)
        shared["Wh"], shared["bh"] = _poison(tied["Wh"], 0), _poison(tied["bh"], 0)
        for form in (0, 1, 2):
            for whT in (False, True):
                want = HK.run_policy(tied, form, whT)
                with _shared():
                    got = HK.run_policy(shared, form, whT)
                for k in ("a", "a2", "logpi", "cache"):
                    assert _same(got[k], want[k]), (A, W, form, whT, k)


@pytest.mark.parametrize("E", [1, 3])
def test_shared_critic_head_is_the_tied_multi_head_critic_head(E):
    for W in (4, 6, 260):
        base = C.critic_case(E, W, (5, 17, 3))
        tied = dict(base)
        for k in ("Wh", "bh", "tWh", "tbh"):
            tied[k] = np.ascontiguousarray(np.repeat(base[k][:, :1], base["T_l"], axis=1))
        shared = dict(tied)
        for k in ("Wh", "bh", "tWh", "tbh"):
            shared[k] = _poison(tied[k], 1)
        for mode, fused in ((0, False), (1, False), (1, True), (2, False)):
            want = HK.run_critic(tied, mode, fused)
            with _shared():
                got = HK.run_critic(shared, mode, fused)
            for k in ("y_out", "dq", "row_a", "row_b", "alpha_w"):
                assert _same(got[k], want[k]), (E, W, mode, fused, k)


@pytest.mark.parametrize("hd", [1, 8, 12])
def test_shared_data_grad_reads_block_zero_only(hd):
    """mtsac_debug_head_backward under the shared switch (planes included) against T tied heads, the other blocks NaN."""
    for W in (4, 260):
        E = 2 if hd == 1 else 1
        base = C.backward_case(hd, E, W, (5, 17, 3))
        tied = dict(base)
        tied["Wh"] = np.ascontiguousarray(np.repeat(base["Wh"][:, :1], base["T_l"], axis=1))
        shared = dict(tied)
        shared["Wh"] = _poison(tied["Wh"], 1)
        for planes in (0, 3):
            want = HK.run_backward(tied, 0, planes)
            with _shared():
                got = HK.run_backward(shared, 0, planes)
            for k in ("dz", "db", "dbp", "planes", "dWh", "dbh"):
                assert _same(got[k], want[k]), (hd, W, planes, k)
        with _shared():
            both = HK.run_backward(shared, 1)
        assert both["ran"] == 0, "head_backward_both must refuse a shared head (its weight grad is per task)"
