"""The wide head kernels (mtrl_amd/csrc/heads_wide.h: actor heads of hd = 2A > 8, A = 5 .. 64) one by one, through
the mtsac_debug_head_* entry points and the launch wrappers, against the float64 statements of
tests/sac_head_ref.py with the bars of tests/sac_head_wide_bounds.py (every c derived there from the order the
kernels document).  A = 5, 8, 19, 33, 64 put hd = 10, 16, 38, 66, 128 on both sides of the 16-wide output tile
and of a 64-wide one and include the maximum; W = 4 .. 516 all multiples of 4; tasks of 0 .. 257 rows, with 15 /
16 / 17 and 33 rows for the 16-row tile edge.  Buffers are NaN-prefilled between guard bands (the wrappers of
tests/test_gpu_head_kernels.py), every element is compared, the bitwise promises on the raw words."""

from __future__ import annotations

import numpy as np
import pytest

import sac_head_bounds as Bd
import sac_head_cases as C
import sac_head_ref as R
import sac_head_wide_bounds as Wb
import test_gpu_head_kernels as K

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
WIDTHS = K.W_VEC
COUNTS = K.COUNTS + [(15, 16, 17), (33,)]
A_WIDE = [5, 8, 19, 33, 64]
PARTS = K.PARTS
_same = K._same


def _subset(c, idx, keys, axis):
    """The case restricted to (or permuted by) the batch rows idx."""
    d = dict(c)
    for k in keys:
        d[k] = np.ascontiguousarray(np.take(c[k], idx, axis=axis[k] if isinstance(axis, dict) else axis))
    d["task"] = np.ascontiguousarray(c["task"][idx])
    d["B"] = len(idx)
    return d


# ------------------------------------------------------------------ policy head
@pytest.mark.parametrize("A", A_WIDE)
def test_wide_policy_head(A):
    """The rollout form against the reference; the grouped and pair forms, with and without WhT and at every
    rows-per-wave setting, bitwise equal to it; a row's outputs the same whichever rows share its launch."""
    worst, spreads = {}, {k: 0.0 for k in K.TAIL_SPREAD}
    for i, W in enumerate(WIDTHS):
        c = C.policy_case(A, W, COUNTS[(i + A) % len(COUNTS)])
        B, T_l = c["B"], c["T_l"]
        exp = [Wb.policy_expect(c, s) for s in range(2)]
        for _, _, sp in exp:
            for k, v in sp.items():
                spreads[k] = max(spreads[k], float(v))
        base = K.run_policy(c, 0)
        K._policy_compare(c, base, 0, exp[0][0], exp[0][1], worst)
        pair1 = None
        for whT in (False, True):
            variants = [("row", K.run_policy(c, 0, whT)), ("grouped", K.run_policy(c, 1, whT)), ("pair", K.run_policy(c, 2, whT))]
            if not whT:
                for rw in (1, 2, 4):  # the wide kernels take 16-row tiles whatever the setting: the same bits
                    with K._rw(rw):
                        variants.append((f"grouped rw{rw}", K.run_policy(c, 1, whT)))
            for name, got in variants:
                for k in ("a", "a2", "logpi", "cache"):
                    assert _same(got[k][0], base[k][0]), (name, whT, k, "differs bitwise from the per-row launch", W)
                if name == "pair":
                    if pair1 is None:
                        pair1 = got
                        K._policy_compare(c, got, 1, exp[1][0], exp[1][1], worst)
                    for k in ("a", "a2", "logpi", "cache"):
                        assert _same(got[k][1], pair1[k][1]), (name, whT, k, "second row set differs bitwise", W)
        # row independence: one task at a time, and the batch rows permuted
        keys, axis = ("h", "eps"), 1
        for t in range(T_l):
            idx = np.flatnonzero(c["task"] == t)
            if len(idx) == 0 or len(idx) == B:
                continue
            got = K.run_policy(_subset(c, idx, keys, axis), 1, True)
            for k in ("a", "logpi", "cache"):
                assert _same(got[k][0], base[k][0][idx]), (W, t, k, "a task's rows change with the other tasks' rows")
        perm = np.random.default_rng(W + A).permutation(B)
        got = K.run_policy(_subset(c, perm, keys, axis), 1, False)
        for k in ("a", "logpi", "cache"):
            assert _same(got[k][0], base[k][0][perm]), (W, k, "a row's outputs change with its place in the batch")
        for planes, form, rel, floor in ((3, 1, 2.0 ** -23, 2.0 ** -133), (2, 2, 2.0 ** -21, 2.0 ** -38)):
            got = K.run_policy(c, form, True, planes)
            for s in range(2 if form == 2 else 1):
                ps, av = got["planes"][s], got["a"][s][:, :A].astype(f64)
                assert np.isnan(ps[:, A:]).all(), "plane columns past A were written"
                assert R.within(ps[:, :A], av, rel * np.abs(av) + floor), (planes, s, W)
                assert _same(got["a"][s], (base if s == 0 else pair1)["a"][s])
    print(f"wide policy head A={A}: c_dot_wide up to {Wb.c_dot_wide(516)}, spreads {spreads}, worst err / bound {worst}")


# ------------------------------------------------------------------ head backward
@pytest.mark.parametrize("A", A_WIDE)
def test_wide_head_backward(A):
    """The data and weight passes against the reference, without planes and with split3 / split2h planes;
    head_backward_both bitwise equal to the separate passes; rows independent of their launch."""
    hd, worst = 2 * A, {}
    for i, W in enumerate(WIDTHS):
        E = 1 + (i + A) % 2
        counts = COUNTS[(i + 2 * A + 1) % len(COUNTS)]
        c = C.backward_case(hd, E, W, counts)
        T_l, B = c["T_l"], c["B"]
        want, bnd, _ = Wb.backward_expect(c)
        n_t = np.array(counts)
        base = {}
        for planes in (0, 3, 2):
            got = K.run_backward(c, 0, planes)
            base[planes] = got
            assert got["ran"] == 1
            for k in ("dz", "db", "dbp", "dWh", "dbh"):
                if planes:
                    assert _same(got[k], base[0][k]), (W, planes, k, "changes with the plane format")
                    continue
                assert R.within(got[k], want[k], bnd[k]), (W, hd, E, k, "worst err / bound", R.worst(got[k], want[k], bnd[k]))
                worst[k] = max(worst.get(k, 0.0), R.worst(got[k], want[k], bnd[k]))
            for t in np.flatnonzero(n_t == 0):  # an empty task: exact zeros
                assert (got["dWh"][:, t] == 0).all() and (got["dbh"][:, t] == 0).all()
                assert (got["dbp"][:, 4 * t:4 * t + 4] == 0).all()
            if planes:
                dzv = got["dz"].astype(f64)
                tol = 2.0 ** -23 * np.abs(dzv) + 2.0 ** -133 if planes == 3 else 2.0 ** -21 * np.abs(dzv) + 2.0 ** (-24 - got["ec"])
                assert R.within(got["planes"], dzv, tol), (W, hd, planes)
                if planes == 2:  # the exponent holds the bound hd max|dout| max|Wh| below 2^15
                    bound = hd * float(np.abs(c["dout"]).max()) * float(np.abs(c["Wh"]).max())
                    assert bound * 2.0 ** got["ec"] < 2.0 ** 15 and (bound == 0 or bound * 2.0 ** got["ec"] >= 2.0 ** 13)
            else:
                assert np.isnan(got["planes"]).all()
            both = K.run_backward(c, 1, planes)
            assert both["ran"] == 1
            for k in ("dz", "db", "dbp", "dWh", "dbh", "planes"):
                assert _same(both[k], got[k]), (W, hd, planes, k, "differs bitwise from the separate passes")
        keys, axis = ("h", "dout"), 1
        for t in range(T_l):  # one task at a time: its rows, its slices, its head's grads
            idx = np.flatnonzero(c["task"] == t)
            if len(idx) == 0 or len(idx) == B:
                continue
            got = K.run_backward(_subset(c, idx, keys, axis), 0, 0)
            assert _same(got["dz"], base[0]["dz"][:, idx]), (W, t, "dz changes with the other tasks' rows")
            for k, sl in (("dWh", slice(t, t + 1)), ("dbh", slice(t, t + 1)), ("dbp", slice(4 * t, 4 * t + 4))):
                assert _same(got[k][:, sl], base[0][k][:, sl]), (W, t, k, "a task's sums change with the other tasks")
        perm = np.random.default_rng(W + A).permutation(B)
        got = K.run_backward(_subset(c, perm, keys, axis), 0, 3)
        assert _same(got["dz"], base[0]["dz"][:, perm]) and _same(got["planes"], base[3]["planes"][:, perm]), (
            W, "a row's data grad changes with its place in the batch")
    print(f"wide head backward hd={hd}: c dz {Wb.c_dz_wide(hd)}, colsum up to {Wb.c_colsum_wide(257, 5)}, wgrad / bgrad up "
          f"to {Wb.c_wgrad_wide(257)}; worst err / bound {worst}")


# ------------------------------------------------------------------ action grad
AG_B = [1, 5, 17, 65, 257, 4, 16, 33]


@pytest.mark.parametrize("A", A_WIDE)
def test_wide_action_grad(A):
    """slot and a_data null and given, E = 1, 2, 4.  A = 5 and 8 run action_grad_kernel's AM = 8 instance (the
    narrow kernels' bars), A > 8 the wide kernel (16 rows per workgroup, one max |dout| each)."""
    worst, wide = {}, A > 8
    for i, Wc in enumerate(WIDTHS):
        E, B = (1, 2, 4)[(i + A) % 3], AG_B[(i + A) % len(AG_B)]
        c = C.action_grad_case(A, E, Wc, B)
        for a_data in (False, True):
            r, bnd = (Wb if wide else Bd).action_grad_expect(c, a_data)
            base = None
            for slot in (False, True):
                got = K.run_action_grad(c, slot, a_data)
                rows_wg = 16 if wide else None  # a workgroup's rows: its one max |dout|
                if wide:
                    parts = min(-(-B // 16), PARTS)
                    assert got["parts"] == parts and np.isnan(got["amax"][parts:]).all()
                    mx = np.zeros(parts, f32)
                    np.maximum.at(mx, (np.arange(B) // rows_wg) % parts, np.abs(got["dout"]).max(1))
                    assert _same(got["amax"][:parts], mx), (Wc, "max |dout| partials")
                if base is None:
                    base = got
                    assert R.within(got["dout"], r["dout"], bnd["dout"]), (A, E, Wc, B, a_data, "worst err / bound",
                                                                           R.worst(got["dout"], r["dout"], bnd["dout"]))
                    worst["dout"] = max(worst.get("dout", 0.0), R.worst(got["dout"], r["dout"], bnd["dout"]))
                    if a_data:
                        assert R.within(got["row_explore"], r["row_explore"], bnd["row_explore"]), (A, Wc, B)
                        assert R.within(got["row_loss"], r["row_loss"], bnd["row_loss"]), (A, Wc, B)
                        assert got["row_explore"][0] == 0, "a_data == a in row 0: its explore term is exactly 0"
                    else:
                        assert np.isnan(got["row_loss"]).all() and np.isnan(got["row_explore"]).all()
                for k in ("dout", "row_loss", "row_explore"):
                    assert _same(got[k], base[k]), (A, E, Wc, B, a_data, slot, k, "differs bitwise")
            if B > 1:  # a row's gradient does not depend on its place in the batch
                perm = np.random.default_rng(Wc + A).permutation(B)
                d = dict(c)
                for k, ax in (("dz1", 1), ("dq", 1), ("cache", 0), ("alpha_w", 0), ("a_data", 0), ("row_loss", 0)):
                    d[k] = np.ascontiguousarray(np.take(c[k], perm, axis=ax))
                got = K.run_action_grad(d, True, False)
                ref = K.run_action_grad(c, True, False)
                assert _same(got["dout"], ref["dout"][perm]), (A, E, Wc, B, "a row's dout changes with its place")
    print(f"action grad A={A}: c up to {Wb.c_agrad_wide(516, 4) if wide else R.c_agrad(516, 4)}, worst err / bound {worst}")


# ------------------------------------------------------------------ dispatch refusals
def _z(n=1 << 12):
    return np.zeros(n, f32)


def _zi(n=64):
    return np.zeros(n, np.int32)


def _bwd_rc(hd, W):
    """The backward entry point on one zero row of one task: every output its own buffer."""
    outs = [_z() for _ in range(6)]
    return K._lib().mtsac_debug_head_backward(0, 0, 1, 1, 1, W, hd, K._p(_zi()), K._p(_z()), K._p(_z()), K._p(_z()), None,
                                              *[K._p(o) for o in outs], K._p(_zi()), K._p(_zi()), K._p(_zi()))


def test_uncovered_head_width_is_refused():
    """hd = 3 has no kernel: an error, not another width's kernel."""
    assert _bwd_rc(3, 4) == -22 and _bwd_rc(5, 4) == -22 and _bwd_rc(7, 4) == -22
    assert _bwd_rc(10, 4) == 0, "the same call at a covered width runs"


def test_wide_head_needs_width_multiple_of_4():
    """W = 6 at hd = 10: the wide kernels have no scalar-W path, the entry points say so."""
    assert _bwd_rc(10, 6) == -22 and _bwd_rc(10, 8) == 0

    def pol(W):
        outs = [_z() for _ in range(4)]
        return K._lib().mtsac_debug_head_policy(0, 0, 1, 1, W, 5, 5, K._p(_zi()), K._p(_z()), K._p(_z()), K._p(_z()),
                                                K._p(_z()), -2.0, 1.0, *[K._p(o) for o in outs], None, K._p(_zi()),
                                                K._p(_zi()))

    assert pol(6) == -22 and pol(8) == 0

    def ag(Wc):
        outs = [_z() for _ in range(4)]
        return K._lib().mtsac_debug_head_action_grad(1, 1, Wc, 24, 19, K._p(_z()), None, K._p(_z()), K._p(_z()), K._p(_z()),
                                                     None, 0, 0.0, -2.0, 1.0, None, *[K._p(o) for o in outs], K._p(_zi()))

    assert ag(6) == -22 and ag(8) == 0


def test_shared_output_buffers_are_refused():
    """Two outputs of a call at one address would be copied back over each other: refused, at any A."""
    P, zi = K._p(_z()), K._p(_zi())
    for A in (2, 5):
        assert K._lib().mtsac_debug_head_policy(0, 0, 1, 1, 8, A, A, K._p(_zi()), K._p(_z()), K._p(_z()), K._p(_z()),
                                                K._p(_z()), -2.0, 1.0, P, P, P, P, None, zi, zi) == -22
        assert K._lib().mtsac_debug_head_action_grad(1, 1, 8, A + 5, A, K._p(_z()), None, K._p(_z()), K._p(_z()),
                                                     K._p(_z()), None, 0, 0.0, -2.0, 1.0, None, P, P, P, P, zi) == -22
