"""The replay kernels of mtrl_amd/csrc/replay.hip one by one (the mtsac_debug_replay_gather / task_rows /
pack_commit / absmax / fill_synthetic entry points of include/mtsac_debug.h) against tests/replay_ref.py.

Every device output starts as NaN (-1 for ints, 0xFFFF for plane words) between two guard bands, and every
element is compared on its raw bits: what a kernel must leave alone (pad columns, the action columns of xc_pi /
xc_next and of their planes, plane rows between the two blocks of pa, list entries past a count) has to come
back untouched.  The store's pad floats and every slot that is not sampled hold NaN, so a read of the wrong
record or column shows.  The only tolerance is philox_ref.normal_bound on the synthetic fill's normals; the only
bits not compared are the signs of zero plane words (compare_gather says why)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import replay_ref as RR

pytestmark = pytest.mark.gpu

f32 = np.float32
PV = ctypes.c_void_p


def _lib():
    from mtrl_amd import _lib as L

    return L.load()


def _check(rc):
    from mtrl_amd import _lib as L

    L.check(rc)


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(PV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _where(a, b):
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16) !=
                    np.ascontiguousarray(b).view(np.uint32 if b.dtype.itemsize == 4 else np.uint16))
    return [(i.tolist(), a[tuple(i)].item(), b[tuple(i)].item()) for i in d[:4]]  # (index, got, want)


# ------------------------------------------------------------------ gather / scatter
def make_batch(n, T_l, D, A, T_glob, task_begin, seed):
    """Batch rows (row i T_l + t of local task t) with Gaussian features (one exactly 1.0, one -0.0 one-hot zero)."""
    rng = np.random.default_rng(seed)
    B, F = n * T_l, D - T_glob
    obs, nobs = np.zeros((B, D), f32), np.zeros((B, D), f32)
    obs[:, :F], nobs[:, :F] = rng.standard_normal((B, F)), rng.standard_normal((B, F))
    t = np.arange(B) % T_l
    obs[np.arange(B), F + task_begin + t] = nobs[np.arange(B), F + task_begin + t] = 1
    if F > 0:
        obs[0, 0] = 1.0  # a feature equal to 1.0 is no one-hot entry
    if T_glob > 1:  # a -0.0 among the one-hot zeros is accepted
        obs[B - 1, F + (task_begin + t[B - 1] + 1) % T_glob] = -0.0
    act = rng.uniform(-1, 1, (B, A)).astype(f32)
    rew, done = rng.uniform(-5, 10, B).astype(f32), (rng.uniform(size=B) < 0.3).astype(f32)
    return obs, act, nobs, done, rew


def run_gather(batch, n, T_l, T_glob, task_begin, ld_a, ld_c, plane_mode=0, in_max=None, norm=None, from_store=True,
               seed=0, double=True):
    """The launch and the model on the same rows -> (got, want)."""
    obs, act, nobs, done, rew = batch
    B, D = obs.shape
    A = act.shape[1]
    R = RR.record_width(D, A) + (4 if seed % 2 else 0)  # a wider record stride is allowed
    pa_ld, pc_ld = (D + 7) // 8 * 8, (A + D + 7) // 8 * 8 + 8
    pa_next, pa_rows, pc_rows = B + 3, 2 * B + 5, B + 2
    np_ = 2 if plane_mode == 2 else 3
    store = idx = None
    if from_store:
        cap = n + 5
        idx = np.random.default_rng(seed).permutation(cap)[:n].astype(np.int32)
        if n > 1 and double:
            idx[-1] = idx[0]  # a slot sampled twice
            obs, act, nobs, done, rew = (x.copy() for x in (obs, act, nobs, done, rew))
            for x in (obs, act, nobs, done, rew):
                x.reshape((n, T_l) + x.shape[1:])[-1] = x.reshape((n, T_l) + x.shape[1:])[0]
        store = np.full((cap, T_l, R), np.nan, f32)  # unsampled slots and the pad: NaN
        rec = RR.pack_records(obs, act, rew, done, nobs, R, pad=np.nan).reshape(n, T_l, R)
        store[idx] = rec
    dims = np.array([0 if from_store else 1, n if from_store else B, T_l, 0 if store is None else store.shape[0], D, A,
                     T_glob, task_begin, ld_a, ld_c, plane_mode, pa_ld, pc_ld, pa_next, pa_rows, pc_rows, R], np.int32)
    o = dict(xa=np.zeros((B, ld_a), f32), xa_next=np.zeros((B, ld_a), f32), xc=np.zeros((B, ld_c), f32),
             xc_next=np.zeros((B, ld_c), f32), xc_pi=np.zeros((B, ld_c), f32), rew=np.zeros(B, f32), done=np.zeros(B, f32),
             task=np.zeros(B, np.int32), err=np.zeros(1, np.int32))
    if plane_mode:
        o["pa"] = np.zeros((np_, pa_rows, pa_ld), np.uint16)
        for k in ("pc", "pcn", "pcp"):
            o[k] = np.zeros((np_, pc_rows, pc_ld), np.uint16)
    e = np.full(1, -777, np.int32)
    rmin, rmax, eps = norm if norm is not None else (None, None, 0.0)
    im = None if in_max is None else np.array([in_max], f32)
    user = [None] * 5 if from_store else [np.ascontiguousarray(x, f32) for x in (obs, act, nobs, done, rew)]
    _check(_lib().mtsac_debug_replay_gather(
        _p(dims), _p(store), _p(idx), *[_p(u) for u in user], _p(rmin), _p(rmax), eps, _p(im), _p(o["xa"]),
        _p(o["xa_next"]), _p(o["xc"]), _p(o["xc_next"]), _p(o["xc_pi"]), _p(o["rew"]), _p(o["done"]), _p(o["task"]),
        _p(o["err"]), _p(o.get("pa")), _p(o.get("pc")), _p(o.get("pcn")), _p(o.get("pcp")),
        _p(e) if plane_mode == 2 else None))
    o["err"] = int(o["err"][0])
    if plane_mode == 2:
        o["e"] = int(e[0])
    want = RR.gather_model(obs, act, nobs, done, rew, T_l, T_glob, task_begin, ld_a, ld_c, plane_mode, pa_ld, pc_ld,
                           pa_next, pa_rows, pc_rows, in_max, rmin if from_store else None, rmax, eps)
    return o, want


def compare_gather(got, want, tag):
    for k, w in want.items():
        if k in ("pa", "pc", "pcn", "pcp"):
            # the sign of a zero word is not part of the plane format (the GEMMs read h + l, and +-0 adds exactly 0
            # to every product sum): the device splits -0.0 into (+0, -0) where the model gives (-0, +0), because its
            # h is one fused fp16(x s + 0), and (-0) s + (+0) is +0
            g = got[k].copy()
            g[g == 0x8000], w = 0, np.where(w == 0x8000, 0, w).astype(np.uint16)
            assert _same(g, w), (tag, k, "first differing elements", _where(g, w))
        elif isinstance(w, np.ndarray):
            assert _same(got[k], w), (tag, k, "first differing elements", _where(got[k], w))
        else:
            assert got[k] == w, (tag, k, got[k], w)


# (D, A, T_l, T_glob, task_begin, n): D on both sides of the 64-lane column loop's one, two and three rounds,
# A = 1 .. 64, B = n T_l odd and not a multiple of the 4 rows per block, a task shard inside a wider one-hot
SHAPES = [
    (5, 1, 1, 1, 0, 1),
    (5, 4, 3, 4, 1, 3),
    (64, 6, 3, 10, 7, 3),
    (65, 4, 1, 3, 2, 7),
    (89, 4, 3, 50, 20, 3),
    (89, 64, 64, 80, 16, 1),
    (130, 6, 64, 80, 5, 2),
    (130, 1, 3, 80, 77, 5),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d_A%d_T%d_G%d_tb%d_n%d" % s)
def test_gather_and_scatter(shape):
    D, A, T_l, T_glob, tb, n = shape
    batch = make_batch(n, T_l, D, A, T_glob, tb, seed=D + A)
    ld_a, ld_c = D + 3, A + D + 5
    rng = np.random.default_rng(D)
    rmin = rng.uniform(-6, -5, T_l)
    norm = (rmin, rmin + rng.uniform(0.5, 20, T_l), 1e-8)
    for from_store in (True, False):
        for plane_mode, in_max in ((0, None), (1, None), (2, 0.3), (2, 37.5)):
            got, want = run_gather(batch, n, T_l, T_glob, tb, ld_a, ld_c, plane_mode, in_max,
                                   norm if plane_mode == 1 else None, from_store, seed=D + plane_mode)
            compare_gather(got, want, (shape, from_store, plane_mode, in_max))
            assert want["err"] == 0 and np.array_equal(want["task"], np.arange(n * T_l) % T_l)
    # dense widths: no pad column at all
    got, want = run_gather(batch, n, T_l, T_glob, tb, D, A + D, 0, None, norm, True, seed=1)
    compare_gather(got, want, (shape, "dense"))


def _break(batch, row, kind, D, T_glob, tb, T_l):
    obs, act, nobs, done, rew = (x.copy() for x in batch)
    F = D - T_glob
    cur = F + int(np.argmax(obs[row, F:] == 1))
    other = F + tb + ((cur - F - tb) + 1) % T_l if T_l > 1 else None
    if kind == "zeros":
        obs[row, F:] = 0
    elif kind == "two":
        obs[row, F + (cur - F + 1) % T_glob] = 1
    elif kind == "two_next":
        nobs[row, F + (cur - F + 1) % T_glob] = 1
    elif kind == "half":
        nobs[row, F + (cur - F + 1) % T_glob] = 0.5
    elif kind == "nan":
        obs[row, F + (cur - F + 1) % T_glob] = np.nan
    elif kind == "differ":
        nobs[row, cur], nobs[row, other] = 0, 1
    elif kind == "below":
        obs[row, cur] = nobs[row, cur] = 0
        obs[row, F + tb - 1] = nobs[row, F + tb - 1] = 1
    elif kind == "above":
        obs[row, cur] = nobs[row, cur] = 0
        obs[row, F + tb + T_l] = nobs[row, F + tb + T_l] = 1
    elif kind == "negzero":
        z = F + (cur - F + 1) % T_glob
        obs[row, z] = nobs[row, z] = -0.0
    elif isinstance(kind, tuple):  # ("col", c): a second one at column c of the row
        which, c = kind
        (obs if which == "col" else nobs)[row, c] = 1
    return obs, act, nobs, done, rew


def test_one_hot_failures():
    """Each broken row sets err and gets task 0, alone; the other rows keep their tasks.  D = 130, T_glob = 80:
    the one-hot spans columns 50 .. 129, so lanes' second and third rounds (columns 64 .., 128 ..) hold part."""
    D, A, T_l, T_glob, tb, n = 130, 4, 3, 80, 40, 3
    base = make_batch(n, T_l, D, A, T_glob, tb, seed=3)
    B = n * T_l
    kinds = ["zeros", "two", "two_next", "half", "nan", "differ", "below", "above"]
    kinds += [("col", c) for c in (50, 63, 64, 65, 127, 128, 129)] + [("ncol", c) for c in (63, 64, 128)]
    for i, kind in enumerate(kinds):
        row = (2 * i + 1) % B  # task of the row is row % T_l: rows of task 1 and 2 show the reset to 0
        if row % T_l == 0:
            row += 1
        for from_store in (True, False):
            got, want = run_gather(_break(base, row, kind, D, T_glob, tb, T_l), n, T_l, T_glob, tb, D + 2, A + D + 2,
                                   from_store=from_store, seed=i, double=False)
            assert want["err"] == 1 and want["task"][row] == 0 and (np.delete(want["task"], row) == np.delete(np.arange(B) % T_l, row)).all(), kind
            compare_gather(got, want, (kind, row, from_store))
    got, want = run_gather(_break(base, 4, "negzero", D, T_glob, tb, T_l), n, T_l, T_glob, tb, D + 2, A + D + 2, from_store=False)
    assert want["err"] == 0
    compare_gather(got, want, "negzero")
    got, want = run_gather(base, n, T_l, T_glob, tb, D + 2, A + D + 2)
    assert want["err"] == 0 and got["err"] == 0


# ------------------------------------------------------------------ task_rows
def run_task_rows(task, T_l, max_rows):
    task = np.ascontiguousarray(task, np.int32)
    counts, rows = np.zeros(T_l, np.int32), np.zeros((T_l, max_rows), np.int32)
    _check(_lib().mtsac_debug_task_rows(len(task), T_l, max_rows, _p(task), _p(counts), _p(rows)))
    return counts, rows


@pytest.mark.parametrize("B", [1, 5, 255, 256, 257, 1000])
def test_task_rows(B):
    rng = np.random.default_rng(B)
    for T_l in (1, 3, 64):
        mixes = dict(random=rng.integers(0, T_l, B), one=np.full(B, T_l - 1), sparse=rng.choice([0, T_l // 2, T_l - 1], B),
                     interleaved=np.arange(B) % T_l)
        for name, task in mixes.items():
            n_t = np.bincount(task, minlength=T_l)
            for max_rows in {B, max(1, int(n_t.max()) - 1), max(1, int(n_t.max()) // 2)}:
                counts, rows = run_task_rows(task, T_l, max_rows)
                wc, wr = RR.task_rows_model(task, T_l, max_rows)
                assert np.array_equal(counts, wc), (B, T_l, name, max_rows)
                assert np.array_equal(rows, wr), (B, T_l, name, max_rows, np.argwhere(rows != wr)[:4].tolist())


# ------------------------------------------------------------------ pack / commit / absmax
def run_pack_commit(obs, nobs, act, rew, done, R, size, rmin, rmax, bufmax):
    T_l, D = obs.shape
    A = act.shape[1]
    rec = np.zeros((T_l, R), f32)
    mn, mx = (None, None) if rmin is None else (rmin.copy(), rmax.copy())
    bs, bm = np.full(1, -9, np.int64), None if bufmax is None else np.array([bufmax], f32)
    _check(_lib().mtsac_debug_pack_commit(T_l, D, A, R, size, _p(obs), _p(nobs), _p(act), _p(rew), _p(done), _p(rec),
                                          _p(mn), _p(mx), _p(bs), _p(bm)))
    return rec, mn, mx, int(bs[0]), None if bm is None else bm[0]


@pytest.mark.parametrize("T_l,D,A", [(64, 89, 4), (1, 5, 1), (3, 130, 64), (7, 42, 6)])
def test_pack_and_commit(T_l, D, A):
    rng = np.random.default_rng(T_l + D)
    R = RR.record_width(D, A)
    rmin, rmax = np.full(T_l, np.inf), np.full(T_l, -np.inf)
    bufmax = f32(0.0)
    plans = ["plain", "big_reward_done", "last_action", "last_next_obs", "small", "plain"]
    for k, plan in enumerate(plans):
        obs, nobs = rng.standard_normal((T_l, D)).astype(f32), rng.standard_normal((T_l, D)).astype(f32)
        act = rng.uniform(-1, 1, (T_l, A)).astype(f32)
        rew, done = rng.uniform(-3, 9, T_l).astype(f32), (rng.uniform(size=T_l) < 0.5).astype(f32)
        if plan == "big_reward_done":
            rew[-1], done[0] = 1e6, 2e6  # neither may reach bufmax
        if plan == "last_action":
            act[-1, -1] = -50.0
        if plan == "last_next_obs":
            nobs[-1, -1] = 70.0
        if plan == "small":
            obs, nobs, act = obs * f32(0.01), nobs * f32(0.01), act * f32(0.01)  # bufmax never decreases
        rec, mn, mx, bs, bm = run_pack_commit(obs, nobs, act, rew, done, R, 1000 + k, rmin, rmax, bufmax)
        wrec, wmn, wmx, wbm = RR.pack_commit_model(obs, nobs, act, rew, done, R, rmin, rmax, bufmax)
        assert _same(rec, wrec), (plan, _where(rec, wrec))
        assert np.array_equal(mn, wmn) and np.array_equal(mx, wmx), plan
        assert bs == 1000 + k and _same(np.array([bm]), np.array([wbm])), (plan, bm, wbm)
        assert bm >= bufmax and bm < 1e5
        rmin, rmax, bufmax = mn, mx, bm
    assert bufmax == 70.0
    # without reward statistics and without a bound: the record and the size alone
    rec, mn, mx, bs, bm = run_pack_commit(obs, nobs, act, rew, done, R + 4, 5, None, None, None)
    assert _same(rec, RR.pack_records(obs, act, rew, done, nobs, R + 4)) and bs == 5


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_absmax(n):
    x = np.random.default_rng(n).standard_normal(n).astype(f32)
    for place, m0 in ((n - 1, 0.5), (0, 0.5), (n // 2, 0.5), (n - 1, 1e3)):
        y = x.copy()
        y[place] = -40.0
        m = np.array([m0], f32)
        _check(_lib().mtsac_debug_absmax(n, _p(y), _p(m)))
        assert m[0] == RR.absmax_model(y, m0) == max(40.0, m0), (n, place, m0)


# ------------------------------------------------------------------ synthetic fill
@pytest.mark.parametrize("cap,T_l,D,A,T_glob,tb", [(5, 3, 12, 3, 5, 1), (2, 2, 9, 4, 3, 0), (70, 4, 15, 19, 6, 2)])
def test_fill_synthetic(cap, T_l, D, A, T_glob, tb):
    seed = 0x1234567800000000 + D
    R = RR.record_width(D, A)
    store, bm = np.zeros((cap, T_l, R), f32), np.array([0.25], f32)
    _check(_lib().mtsac_debug_fill_synthetic(cap, T_l, D, A, T_glob, tb, seed, _p(store), _p(bm)))
    want, bound, exact = RR.fill_model(cap, T_l, D, A, T_glob, tb, seed)
    assert _same(store[..., exact], want[..., exact].astype(f32)), _where(store[..., exact], want[..., exact].astype(f32))
    err = np.abs(store[..., ~exact].astype(np.float64) - want[..., ~exact])
    ratio = float((err / bound[..., ~exact]).max())
    print(f"fill_synthetic normals D={D} A={A}: max err / bound {ratio:.3f}")
    assert np.isfinite(store).all() and ratio <= 1.0, ratio
    # the bound of the stored rows: exactly the max of what was stored, which is the model's max to the noise bound
    assert bm[0] == f32(max(0.25, RR.stored_absmax(store, D, A)))
    assert abs(float(bm[0]) - max(0.25, RR.stored_absmax(want, D, A))) <= bound.max()  # |max a - max b| <= max |a - b|
    big = np.array([99.0], f32)
    _check(_lib().mtsac_debug_fill_synthetic(cap, T_l, D, A, T_glob, tb, seed, _p(store), _p(big)))
    assert big[0] == 99.0
