"""The SAC head kernels of mtrl_amd/csrc/heads.hip one by one (the mtsac_debug_head_* entry points of
include/mtsac_debug.h, which go through the launch wrappers of kernels.h) against the plain float64
statements of tests/sac_head_ref.py, on the inputs of tests/sac_head_cases.py: every actor head width
hd = 2, 4, 6, 8 (A = 1..4), the critic's hd = 1 with E = 1..4 members, W = 4, 252, 256, 260, 516 (16-byte
paths) and 6, 70, 130 (scalar paths), 1 / 3 / 5 tasks with 0 .. 257 rows each, interleaved.

Every device output starts as NaN (-1 for ints) between two guard bands: an element a kernel leaves alone
comes back NaN, a store outside the buffer fails the call (-5).  Every element is compared.

Tolerances (sac_head_ref.py states the rule and derives every c):
 * sums: c 2^-24 S per element, c from the kernel's documented order.  The largest of each kind over these
   shapes: head dot product 19 (W = 516), data grad 2 hd = 16, its column sums 17 + 3 + 4 T_l = 40 (n = 257,
   T_l = 5), weight grad 69 (n = 257), bias grad 10, action grad 4 x 12 + 6 = 54 (E = 4, Wc = 516).
 * transcendental tails: TAIL_FACTOR = 4 times the spread between a float32 numpy evaluation of the reference
   and the float64 one on the same inputs, relative to each element's scale.  TAIL_SPREAD records the largest
   spread measured over all the policy cases of this module (the test asserts it is not exceeded, so the
   record stays true); the factor covers device libm against numpy's float32 routines, an ulp or two each way
   per call, four calls chained per action dimension in logpi.
 * the bitwise equalities heads.hip promises are asserted on the raw words."""

from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

import sac_head_bounds as Bd
import sac_head_cases as C
import sac_head_ref as R

pytestmark = pytest.mark.gpu

U, LIBM = R.U, R.LIBM_ULP
# measured on the policy cases below (float32 numpy evaluation against float64, relative to the element's scale:
# sigma itself, |mu| + |sigma eps| for x, 1 for a, the sum of |terms| for logpi)
TAIL_SPREAD = dict(sigma=2.1e-7, x=1.9e-7, a=3.7e-7, logpi=1.2e-7)
W_VEC, W_SCALAR = (4, 252, 256, 260, 516), (6, 70, 130)
WIDTHS = W_VEC + W_SCALAR
COUNTS = [(5,), (0, 17, 1), (3, 4, 0, 65, 16), (257, 0, 3), (17,), (1, 5, 16, 4, 65), (65, 17, 5), (0, 1, 257, 3, 4)]
PARTS = 2048
f32, f64 = np.float32, np.float64


def _lib():
    from mtrl_amd import _lib as L

    return L.load()


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _in(a, dtype=f32):
    return None if a is None else np.ascontiguousarray(a, dtype)


def _nan(*shape):
    return np.full(shape, np.nan, f32)  # the copy back overwrites it (NaN again where the kernel wrote nothing)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(rc):
    from mtrl_amd import _lib as L

    L.check(rc)


@contextlib.contextmanager
def _rw(rw):
    old = _lib().mtsac_debug_head_rw(rw)
    try:
        yield
    finally:
        _lib().mtsac_debug_head_rw(old)


@contextlib.contextmanager
def _split(mode):
    old = _lib().mtsac_debug_head_bwd_split(mode)
    try:
        yield
    finally:
        _lib().mtsac_debug_head_bwd_split(old)


def _lists_ok(task, T_l, counts, rows):
    want_n, want_rows = R.task_lists(task, T_l)
    assert np.array_equal(counts, want_n), (counts, want_n)
    B = len(task)
    for t in range(T_l):
        assert np.array_equal(rows[t, : want_n[t]], want_rows[t]), t
        assert np.all(rows[t, want_n[t]:] == -1), ("row list written past its count", t)
        assert B >= want_n[t]


# ------------------------------------------------------------------ wrappers
def run_policy(c, form, whT=False, planes=0, pad=3):
    A, B, T_l, W = c["A"], c["B"], c["T_l"], c["W"]
    ns, ld = (2 if form == 2 else 1), A + pad
    h, eps = _in(c["h"][:ns]), _in(c["eps"][:ns])
    o = dict(a=_nan(ns, B, ld), a2=_nan(ns, B, ld), logpi=_nan(ns, B), cache=_nan(ns, B, 5 * A), planes=_nan(ns, B, ld))
    counts, rows = np.zeros(T_l, np.int32), np.zeros((T_l, B), np.int32)
    flags = (1 if whT else 0) | {0: 0, 3: 2, 2: 4}[planes]
    _check(_lib().mtsac_debug_head_policy(form, flags, B, T_l, W, A, ld, _p(c["task"]), _p(h), _p(c["Wh"]), _p(c["bh"]),
                                          _p(eps), C.LS_MIN, C.LS_MAX, _p(o["a"]), _p(o["a2"]), _p(o["logpi"]),
                                          _p(o["cache"]), _p(o["planes"]) if planes else None, _p(counts), _p(rows)))
    _lists_ok(c["task"], T_l, counts, rows)
    return o


def run_critic(c, mode, fused=False, clip=False, tw=False):
    E, B, T_l, W = c["E"], c["B"], c["T_l"], c["W"]
    o = dict(y_out=_nan(B), dq=_nan(E, B), row_a=_nan(B), row_b=_nan(B), alpha_w=_nan(B), amax=_nan(PARTS))
    parts = np.zeros(1, np.int32)
    inv = 1.0 / (E * B) if mode == 1 else 1.0 / B
    _check(_lib().mtsac_debug_head_critic(
        mode, (1 if fused else 0) | (2 if clip else 0), B, T_l, E, W, c["T_glob"], c["task_begin"], _p(c["task"]),
        _p(c["h"]), _p(c["Wh"]), _p(c["bh"]), _p(c["th"]), _p(c["tWh"]), _p(c["tbh"]), _p(c["rew"]), _p(c["done"]),
        _p(c["logpi"]), _p(c["log_alpha"]), _p(c["y"]), _p(c["tw"]) if tw else None, 0.99, inv, _p(o["y_out"]),
        _p(o["dq"]), _p(o["row_a"]), _p(o["row_b"]), _p(o["alpha_w"]), _p(o["amax"]), _p(parts)))
    o["parts"] = int(parts[0])
    return o


def run_backward(c, form, planes=0, compact=False):
    hd, E, B, T_l, W = c["hd"], c["E"], c["B"], c["T_l"], c["W"]
    o = dict(dz=_nan(E, B, W), dbp=_nan(E, 4 * T_l, W), db=_nan(E, W), planes=_nan(E, B, W), dWh=_nan(E, T_l, W, hd),
             dbh=_nan(E, T_l, hd))
    counts, rows, info = np.zeros(T_l, np.int32), np.zeros((T_l, B), np.int32), np.zeros(8, np.int32)
    dq = _in(c["dout"][:, :, 0]) if compact else None
    _check(_lib().mtsac_debug_head_backward(2 if compact else form, {0: 0, 3: 1, 2: 2}[planes], B, T_l, E, W, hd,
                                            _p(c["task"]), _p(c["h"]), _p(c["Wh"]), _p(c["dout"]), _p(dq), _p(o["dz"]),
                                            _p(o["dbp"]), _p(o["db"]), _p(o["planes"]), _p(o["dWh"]), _p(o["dbh"]),
                                            _p(counts), _p(rows), _p(info)))
    _lists_ok(c["task"], T_l, counts, rows)
    assert info[2] == 0, ("head backward self-check fault word", info[2])
    o.update(ran=int(info[0]), ec=int(info[1]), n=info[3:3 + E].copy())
    return o


def run_active_rows(dq):
    E, B = dq.shape
    n, rows, slot = np.zeros(E, np.int32), np.zeros((E, B), np.int32), np.zeros((E, B), np.int32)
    _check(_lib().mtsac_debug_head_active_rows(E, B, _p(_in(dq)), _p(n), _p(rows), _p(slot)))
    return n, rows, slot


def run_action_grad(c, slot=False, a_data=False):
    A, E, B, Wc = c["A"], c["E"], c["B"], c["Wc"]
    o = dict(dout=_nan(B, 2 * A), row_loss=_nan(B), row_explore=_nan(B), amax=_nan(PARTS))
    parts = np.zeros(1, np.int32)
    _check(_lib().mtsac_debug_head_action_grad(
        B, E, Wc, c["Ic"], A, _p(c["dz1"]), _p(c["dq"]) if slot else None, _p(c["W0"]), _p(c["cache"]), _p(c["alpha_w"]),
        _p(c["a_data"]) if a_data else None, c["ld"], float(c["explore_scale"]), C.LS_MIN, C.LS_MAX,
        _p(c["row_loss"]) if a_data else None, _p(o["dout"]), _p(o["row_loss"]), _p(o["row_explore"]), _p(o["amax"]),
        _p(parts)))
    o["parts"] = int(parts[0])
    return o


# ------------------------------------------------------------------ policy head
def _policy_compare(c, got, s, r, bounds, worst):
    A = c["A"]
    a, a2 = got["a"][s], got["a2"][s]
    assert np.isnan(a[:, A:]).all() and np.isnan(a2[:, A:]).all(), "a_out columns past A were written"
    assert _same(a[:, :A], a2[:, :A]) and _same(a[:, :A], got["cache"][s][:, 3 * A:4 * A])
    assert _same(got["cache"][s][:, 4 * A:], c["eps"][s]), "the cache's eps is not the injected one"
    for name, g, want in (("cache", got["cache"][s], r["cache"]), ("a", a[:, :A], r["a"]), ("logpi", got["logpi"][s], r["logpi"])):
        assert R.within(g, want, bounds[name]), (name, s, "worst err / bound", R.worst(g, want, bounds[name]))
        worst[name] = max(worst.get(name, 0.0), R.worst(g, want, bounds[name]))


@pytest.mark.parametrize("A", [1, 2, 3, 4])
def test_policy_head(A):
    """Per row, grouped at 1 / 2 / 4 rows per wave and the pair launch, each with and without WhT: the per-row
    launch against the reference element by element, every other form bitwise equal to it."""
    worst, spreads, seen = {}, {k: 0.0 for k in TAIL_SPREAD}, set()
    for i, W in enumerate(WIDTHS):
        c = C.policy_case(A, W, COUNTS[(i + A) % len(COUNTS)])
        exp = [Bd.policy_expect(c, s) for s in range(2)]
        for _, _, sp in exp:
            for k, v in sp.items():
                spreads[k] = max(spreads[k], float(v))
        base = run_policy(c, 0)
        _policy_compare(c, base, 0, exp[0][0], exp[0][1], worst)
        # the placed edges are there: log-std at a bound (clip factor 0.5), beyond it, saturated tanh, eps 0 / +-4
        ls, a = base["cache"][0][:, A:2 * A], base["a"][0][:, :A]
        seen |= {("ls", v) for v in (C.LS_MIN, C.LS_MAX) if (ls == f32(v)).any()}
        seen |= {("beyond", bool((ls > C.LS_MAX).any() and (ls < C.LS_MIN).any())), ("sat", bool((np.abs(a) == 1).any()))}
        seen |= {("eps", v) for v in (0.0, 4.0, -4.0) if (c["eps"][0] == v).any()}
        pair1 = None
        for whT in (False, True):
            variants = [("row", run_policy(c, 0, whT))]
            for rw in (1, 2, 4):
                with _rw(rw):
                    variants.append((f"grouped rw{rw}", run_policy(c, 1, whT)))
                    variants.append((f"pair rw{rw}", run_policy(c, 2, whT)))
            for name, got in variants:
                for k in ("a", "a2", "logpi", "cache"):
                    assert _same(got[k][0], base[k][0]), (name, whT, k, "differs bitwise from the per-row launch", W)
                if name.startswith("pair"):
                    if pair1 is None:
                        pair1 = got
                        _policy_compare(c, got, 1, exp[1][0], exp[1][1], worst)
                    for k in ("a", "a2", "logpi", "cache"):
                        assert _same(got[k][1], pair1[k][1]), (name, whT, k, "second row set differs bitwise", W)
        # the action planes: their unscaled sum is a, to the planes' precision; columns past A untouched
        for planes, form, rel, floor in ((3, 1, 2.0 ** -23, 2.0 ** -133), (2, 2, 2.0 ** -21, 2.0 ** -38)):
            got = run_policy(c, form, True, planes)
            for s in range(2 if form == 2 else 1):
                ps, av = got["planes"][s], got["a"][s][:, :A].astype(f64)
                assert np.isnan(ps[:, A:]).all(), "plane columns past A were written"
                assert R.within(ps[:, :A], av, rel * np.abs(av) + floor), (planes, s, W)
                assert _same(got["a"][s], (base if s == 0 else pair1)["a"][s])
    for k, v in spreads.items():
        assert v <= TAIL_SPREAD[k], ("measured float32 spread above the recorded one", k, v)
    need = {("ls", C.LS_MIN), ("ls", C.LS_MAX), ("beyond", True), ("sat", True), ("eps", 0.0), ("eps", 4.0), ("eps", -4.0)}
    assert seen >= need - ({("beyond", True)} if A == 1 else set()), seen  # A = 1: beyond the upper bound only
    print(f"policy head A={A}: c_dot up to {R.c_dot(516)}, float32 spreads {spreads}, worst err / bound {worst}")


# ------------------------------------------------------------------ critic head
@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_critic_head(E):
    """All three modes, fused_target, clip and task weights on and off, against the reference; what a mode does
    not write stays untouched; the per-workgroup max |dq| partials."""
    worst, ties, clips = {}, set(), set()
    modes = [(0, False, cl, False) for cl in (False, True)]
    modes += [(1, fu, cl, tw) for fu in (False, True) for cl in (False, True) for tw in (False, True)]
    modes += [(2, False, False, tw) for tw in (False, True)]
    for i, W in enumerate(WIDTHS):
        c = C.critic_case(E, W, COUNTS[(i + E + 3) % len(COUNTS)])
        B = c["B"]
        for mode, fused, clip, tw in modes:
            want, bnd, q, bq = Bd.critic_expect(c, mode, fused, clip, tw)
            got = run_critic(c, mode, fused, clip, tw)
            for k in ("y_out", "dq", "row_a", "row_b", "alpha_w"):
                if k not in want:
                    assert np.isnan(got[k]).all(), (k, "written in mode", mode, fused)
                    continue
                assert R.within(got[k], want[k], bnd[k]), (W, mode, fused, clip, tw, k, "worst err / bound",
                                                           R.worst(got[k], want[k], bnd[k]))
                worst[k] = max(worst.get(k, 0.0), R.worst(got[k], want[k], bnd[k]))
            # one partial max per workgroup, wave w of workgroup g taking row 4 g + w (+ 4 parts k)
            parts = min((B + 3) // 4, PARTS)
            assert got["parts"] == parts
            assert np.isnan(got["amax"][parts:]).all(), "partial maxima past the launcher's count were written"
            mx = np.zeros(parts, f32)
            if mode != 0:
                np.maximum.at(mx, (np.arange(B) // 4) % parts, np.abs(got["dq"]).max(0))
            assert _same(got["amax"][:parts], mx), (W, mode, "max |dq| partials")
            if mode == 2:
                cnt = (q == q.min(0)).sum(0)
                ties |= set(cnt.tolist())
                for n in set(cnt.tolist()):  # a tie of n members: each gets exactly 1 / n of the row's grad
                    rows = np.flatnonzero(cnt == n)
                    nz = (got["dq"][:, rows] != 0).sum(0)
                    assert (nz == n).all(), (W, n)
            if mode == 1 and clip:
                clips |= {"at" if (np.abs(q) == 5000).any() else "", "beyond" if (np.abs(q) > 5000).any() else ""}
    assert ties >= set(range(1, E + 1)), ("tie sizes seen", ties)
    assert clips >= {"at", "beyond"}, clips
    print(f"critic head E={E}: c_dot up to {R.c_dot(516)}, worst err / bound {worst}")


# ------------------------------------------------------------------ head backward
BWD = {"hd2": (2, 0), "hd4": (4, 0), "hd6": (6, 0), "hd8": (8, 0), "hd1-a": (1, 0), "hd1-b": (1, 2)}


@pytest.mark.parametrize("name", list(BWD))
def test_head_backward(name):
    """The data and weight passes against the reference; head_backward_both in both of its forms and every plane
    format bitwise equal to the separate passes; the compacted data pass bitwise equal to the dense rows."""
    hd, rot = BWD[name]
    worst = {}
    for i, W in enumerate(WIDTHS):
        E = 1 + (i + rot) % 4 if hd == 1 else 1
        counts = COUNTS[(i + hd) % len(COUNTS)]
        c = C.backward_case(hd, E, W, counts)
        T_l, B, task = c["T_l"], c["B"], c["task"]
        want, bnd, _ = Bd.backward_expect(c)
        n_t = np.array(counts)
        vec = W % 4 == 0
        base = {}
        for planes in (0, 3, 2):
            got = run_backward(c, 0, planes)
            base[planes] = got
            assert got["ran"] == (1 if vec else 0)
            for k in ("dz", "db", "dbp", "dWh", "dbh"):
                if not vec and k in ("dz", "db", "dbp"):
                    assert np.isnan(got[k]).all(), (k, "written without a data pass")
                    continue
                if planes:
                    assert _same(got[k], base[0][k]), (W, planes, k, "changes with the plane format")
                    continue
                assert R.within(got[k], want[k], bnd[k]), (W, hd, E, k, "worst err / bound", R.worst(got[k], want[k], bnd[k]))
                worst[k] = max(worst.get(k, 0.0), R.worst(got[k], want[k], bnd[k]))
            empty = np.flatnonzero(n_t == 0)
            for t in empty:  # an empty task: exact zeros
                assert (got["dWh"][:, t] == 0).all() and (got["dbh"][:, t] == 0).all()
                assert not vec or (got["dbp"][:, 4 * t:4 * t + 4] == 0).all()
            if planes and vec:  # the planes' unscaled sum is dz, to the planes' precision
                dzv = got["dz"].astype(f64)
                # split3: three bf16 planes hold 24 bits, down to bf16's subnormal spacing 2^-133 (a denormal dz);
                # split2h: two fp16 planes of dz 2^ec hold 22 bits, down to fp16's subnormal spacing 2^-24
                tol = 2.0 ** -23 * np.abs(dzv) + 2.0 ** -133 if planes == 3 else 2.0 ** -21 * np.abs(dzv) + 2.0 ** (-24 - got["ec"])
                assert R.within(got["planes"], dzv, tol), (W, hd, planes)
                if planes == 2:  # the exponent holds the bound hd max|dout| max|Wh| below 2^15
                    bound = hd * float(np.abs(c["dout"]).max()) * float(np.abs(c["Wh"]).max())
                    assert bound * 2.0 ** got["ec"] < 2.0 ** 15 and (bound == 0 or bound * 2.0 ** got["ec"] >= 2.0 ** 13)
            else:
                assert np.isnan(got["planes"]).all()
            for split in (1, 0):
                with _split(split):
                    both = run_backward(c, 1, planes)
                assert both["ran"] == (1 if vec else 0), "head_backward_both must refuse W % 4 != 0"
                for k in ("dz", "db", "dbp", "dWh", "dbh", "planes"):
                    if vec:
                        assert _same(both[k], got[k]), (W, hd, planes, split, k, "differs bitwise from the separate passes")
                    else:
                        assert np.isnan(both[k]).all(), (k, "written by a refused launch")
                assert both["ec"] == got["ec"] or not vec
        if hd == 1 and vec:  # the compacted pass: plane row s of member e = the dense row of its s-th active row
            n, rows, _ = R.active_rows(c["dout"][:, :, 0])
            for planes in (3, 2):
                cp = run_backward(c, 0, planes, compact=True)
                assert np.array_equal(cp["n"], n) and cp["ec"] == base[planes]["ec"]
                for k in ("dz", "db", "dbp", "dWh", "dbh"):
                    assert np.isnan(cp[k]).all(), (k, "written by the compacted pass")
                for e in range(E):
                    assert _same(cp["planes"][e, :n[e]], base[planes]["planes"][e, rows[e, :n[e]]]), (W, E, e, planes)
                    assert np.isnan(cp["planes"][e, n[e]:]).all(), "compacted plane rows past n[e] were written"
    print(f"head backward {name}: c dz {2 * hd}, colsum up to {R.c_colsum(257, 5)}, wgrad up to {R.c_wgrad(257)}, "
          f"bgrad up to {R.c_bgrad(257)}; worst err / bound {worst}")


# ------------------------------------------------------------------ active rows
@pytest.mark.parametrize("B", [1, 63, 64, 1023, 1024, 1025, 2500])
def test_active_rows(B):
    """All active, none, alternating, and random with -0.0 (inactive) and a denormal (active)."""
    rng = np.random.default_rng(B)
    dq = np.zeros((4, B), f32)
    dq[0] = rng.standard_normal(B) + 3
    dq[2, ::2] = -1.0
    dq[2, 1::2] = -0.0
    dq[3] = rng.standard_normal(B) * (rng.uniform(size=B) < 0.5)
    if B > 1:
        dq[3, B - 1] = -0.0
    dq[3, B // 2] = 1e-40
    assert dq[3, B // 2] != 0 and 0 < abs(float(dq[3, B // 2])) < 1.2e-38
    for E in (4, 1):
        n, rows, slot = run_active_rows(dq[4 - E:])
        wn, wrows, wslot = R.active_rows(dq[4 - E:])
        assert np.array_equal(n, wn) and np.array_equal(rows, wrows) and np.array_equal(slot, wslot)
    assert wn[0] == np.count_nonzero(dq[3])


# ------------------------------------------------------------------ action grad
AG_B = [1, 5, 17, 65, 257, 4, 16, 3]


@pytest.mark.parametrize("A", [1, 2, 3, 4])
def test_action_grad(A):
    """slot and a_data null and given, at 1 / 2 / 4 rows per wave: the dense one-row-per-wave launch against the
    reference, every other form bitwise equal to it (A = 4 runs the AM = 4 instance, the others AM = 8)."""
    worst = {}
    for i, Wc in enumerate(WIDTHS):
        E, B = 1 + (i + A) % 4, AG_B[(i + 2 * A) % len(AG_B)]
        c = C.action_grad_case(A, E, Wc, B)
        for a_data in (False, True):
            r, bnd = Bd.action_grad_expect(c, a_data)
            b_dout = bnd["dout"]
            base = None
            for slot in (False, True):
                for rw in (1, 2, 4):
                    with _rw(rw):
                        got = run_action_grad(c, slot, a_data)
                    parts = min((B + 4 * rw - 1) // (4 * rw), PARTS)
                    assert got["parts"] == parts and np.isnan(got["amax"][parts:]).all()
                    mx = np.zeros(parts, f32)
                    np.maximum.at(mx, (np.arange(B) // (4 * rw)) % parts, np.abs(got["dout"]).max(1))
                    assert _same(got["amax"][:parts], mx), (Wc, rw, "max |dout| partials")
                    if base is None:
                        base = got
                        assert R.within(got["dout"], r["dout"], b_dout), (A, E, Wc, B, a_data, "worst err / bound",
                                                                          R.worst(got["dout"], r["dout"], b_dout))
                        worst["dout"] = max(worst.get("dout", 0.0), R.worst(got["dout"], r["dout"], b_dout))
                        if a_data:
                            assert R.within(got["row_explore"], r["row_explore"], bnd["row_explore"]), (A, Wc, B)
                            assert R.within(got["row_loss"], r["row_loss"], bnd["row_loss"]), (A, Wc, B)
                            assert got["row_explore"][0] == 0, "a_data == a in row 0: its explore term is exactly 0"
                        else:
                            assert np.isnan(got["row_loss"]).all() and np.isnan(got["row_explore"]).all()
                    for k in ("dout", "row_loss", "row_explore"):
                        assert _same(got[k], base[k]), (A, E, Wc, B, a_data, slot, rw, k, "differs bitwise")
    print(f"action grad A={A}: c up to {R.c_agrad(516, 4)}, worst err / bound {worst}")


# ------------------------------------------------------------------ row alpha, error paths
@pytest.mark.parametrize("use_tw", [0, 1])
def test_row_alpha(use_tw):
    for T_l, T_glob, begin, B in ((1, 1, 0, 1), (3, 5, 2, 257), (5, 50, 45, 300)):
        rng = np.random.default_rng(T_glob + B)
        task = rng.integers(0, T_l, B).astype(np.int32)
        la = rng.uniform(-3, 3, T_glob).astype(f32)
        alpha, tw = _nan(B), _nan(B)
        _check(_lib().mtsac_debug_head_row_alpha(B, T_l, T_glob, begin, use_tw, _p(task), _p(la), _p(alpha), _p(tw)))
        wa, wt = R.row_alpha(task, begin, la.astype(f64), T_glob)
        assert R.within(alpha, wa, (1 + LIBM) * U * wa)
        if use_tw:  # T_glob exponentials summed in order, a division and two products
            assert R.within(tw, wt, (T_glob + 4 + 2 * LIBM) * U * wt)
        else:
            assert np.isnan(tw).all()


def test_bad_arguments_are_refused():
    lib = _lib()
    z = np.zeros(4096, f32)
    zi = np.zeros(4096, np.int32)
    P = _p(z)
    pol = lambda B, A: lib.mtsac_debug_head_policy(0, 0, B, 1, 4, A, A, _p(zi), P, P, P, P, -2.0, 1.0, P, P, P, P, None,
                                                   _p(zi), _p(zi))
    assert pol(1, 5) == -22 and pol(0, 2) == -22 and pol(1, 0) == -22
    cri = lambda B, E: lib.mtsac_debug_head_critic(2, 0, B, 1, E, 4, 1, 0, _p(zi), P, P, P, None, None, None, P, P, P, P, P,
                                                   None, 0.99, 1.0, P, P, P, P, P, P, _p(zi))
    assert cri(1, 5) == -22 and cri(0, 2) == -22 and cri(1, 0) == -22
    bwd = lambda B, E, hd, W=4, form=0: lib.mtsac_debug_head_backward(form, 0, B, 1, E, W, hd, _p(zi), P, P, P, P, P, P, P, P,
                                                                      P, P, _p(zi), _p(zi), _p(zi))
    assert [bwd(1, 1, hd) for hd in (0, 3, 5, 7, 9)] == [-22] * 5
    assert bwd(1, 5, 1) == -22 and bwd(0, 1, 1) == -22
    assert bwd(1, 1, 2, form=2) == -22 and bwd(1, 1, 1, W=6, form=2) == -22  # the compacted pass: hd = 1, W % 4 == 0
    assert lib.mtsac_debug_head_active_rows(5, 1, P, _p(zi), _p(zi), _p(zi)) == -22
    assert lib.mtsac_debug_head_active_rows(1, 0, P, _p(zi), _p(zi), _p(zi)) == -22
    ag = lambda B, E, A: lib.mtsac_debug_head_action_grad(B, E, 4, 9, A, P, None, P, P, P, None, 0, 0.0, -2.0, 1.0, None, P,
                                                          P, P, P, _p(zi))
    assert ag(1, 1, 5) == -22 and ag(1, 5, 2) == -22 and ag(0, 1, 2) == -22
    assert lib.mtsac_debug_head_row_alpha(0, 1, 1, 0, 0, _p(zi), P, P, P) == -22
    bad_task = np.array([1], np.int32)
    assert lib.mtsac_debug_head_row_alpha(1, 1, 1, 0, 0, _p(bad_task), P, P, P) == -22
    # the setters return the previous override and leave none behind
    assert lib.mtsac_debug_head_rw(2) == -1 and lib.mtsac_debug_head_rw(-1) == 2 and lib.mtsac_debug_head_rw(-1) == -1
    assert lib.mtsac_debug_head_bwd_split(0) == -1 and lib.mtsac_debug_head_bwd_split(-1) == 0
