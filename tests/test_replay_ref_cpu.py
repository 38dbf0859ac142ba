"""tests/replay_ref.py against the oracle's MultiTaskReplayBufferOracle.gather at the shape the engine tests use
(T = 3, D = 42, A = 4, n = 8), and the models' own edge cases."""

import numpy as np

import replay_ref as RR
from oracle.buffer import MultiTaskReplayBufferOracle
from trunk_bias_ref import UNTOUCHED, bf16_words, split2h, split3

f32 = np.float32


def _filled(T, D, A, cap, seed, normalize=False):
    rng = np.random.default_rng(seed)
    orc = MultiTaskReplayBufferOracle(cap * T, T, D, A, seed=1, normalize_rewards=normalize)
    store = np.zeros((cap, T, RR.record_width(D, A)), f32)
    for s in range(cap):
        o = np.zeros((T, D), f32)
        o[:, :D - T] = rng.standard_normal((T, D - T))
        o[np.arange(T), D - T + np.arange(T)] = 1
        no = o.copy()
        no[:, :D - T] = rng.standard_normal((T, D - T))
        a = rng.uniform(-1, 1, (T, A)).astype(f32)
        r, d = rng.uniform(0, 10, T).astype(f32), (rng.uniform(size=T) < 0.2).astype(f32)
        orc.add(o, no, a, r, d)
        store[s] = RR.pack_records(o, a, r, d, no)
    return orc, store


def test_gather_model_matches_oracle():
    T, D, A, n, cap = 3, 42, 4, 8, 16
    for normalize in (False, True):
        orc, store = _filled(T, D, A, cap, 3, normalize)
        idx = orc.sample_indices(n * T)
        obs, act, nobs, done, rew = orc.gather(idx)
        u = RR.unpack_rows(store, idx, D, A)
        kw = dict(rmin=orc._min_rewards, rmax=orc._max_rewards, norm_eps=orc.reward_norm_eps) if normalize else {}
        m = RR.gather_model(*u[:3], u[3], u[4], T, T, 0, 44, 48, **kw)
        B = n * T
        assert np.array_equal(m["xa"][:, :D], obs) and np.array_equal(m["xa_next"][:, :D], nobs)
        assert np.array_equal(m["xc"][:, :A], act) and np.array_equal(m["xc"][:, A:A + D], obs)
        assert np.array_equal(m["xc_pi"][:, A:A + D], obs) and np.array_equal(m["xc_next"][:, A:A + D], nobs)
        assert np.isnan(m["xa"][:, D:]).all() and np.isnan(m["xc"][:, A + D:]).all()
        assert np.isnan(m["xc_pi"][:, :A]).all() and np.isnan(m["xc_next"][:, :A]).all()
        assert np.array_equal(m["done"], done[:, 0])
        assert np.array_equal(m["rew"], rew[:, 0].astype(f32))  # the float64 expression, rounded once
        assert np.array_equal(m["task"], np.arange(B) % T) and m["err"] == 0


def test_one_hot_cases():
    T_glob, tb, T_l, D = 6, 2, 3, 10
    def row(col):
        v = np.zeros(D, f32)
        v[:4] = [0.5, 1.0, -2.0, 0.0]  # feature columns may hold anything, a 1.0 included
        if col is not None:
            v[D - T_glob + col] = 1
        return v
    good = row(3)
    cases = dict(ok=(good, good, 1, 0), zeros=(row(None), good, 0, 1), below=(row(1), row(1), 0, 1),
                 at_end=(row(5), row(5), 0, 1), last_local=(row(4), row(4), 2, 0), differ=(row(2), row(3), 0, 1))
    two = row(3); two[D - 1] = 1
    half = row(3); half[D - T_glob] = 0.5
    nan = row(3); nan[D - 2] = np.nan
    negz = row(3); negz[D - 1] = -0.0
    cases.update(two=(two, good, 0, 1), half=(good, half, 0, 1), nan=(nan, good, 0, 1), negzero=(negz, negz, 1, 0))
    for name, (o, n, task, err) in cases.items():
        t, e = RR.one_hot_task(np.stack([good, o]), np.stack([good, n]), T_glob, tb, T_l)
        assert (t[0], t[1], e) == (1, task, err), name


def test_planes_and_untouched():
    rng = np.random.default_rng(0)
    B, D, A, T = 3, 5, 2, 1
    obs, nobs = rng.standard_normal((B, D)).astype(f32), rng.standard_normal((B, D)).astype(f32)
    obs[:, -1] = nobs[:, -1] = 1
    act = rng.uniform(-1, 1, (B, A)).astype(f32)
    z = np.zeros(B, f32)
    m = RR.gather_model(obs, act, nobs, z, z, T, 1, 0, 8, 8, plane_mode=1, pa_ld=8, pc_ld=8, pa_next=4, pa_rows=8, pc_rows=4)
    h, mid, l = (bf16_words(p) for p in split3(nobs))
    assert np.array_equal(m["pa"][0, 4:7, :D], h) and np.array_equal(m["pa"][2, 4:7, :D], l)
    assert (m["pa"][:, 3] == UNTOUCHED).all() and (m["pa"][:, 7] == UNTOUCHED).all() and (m["pa"][:, :, D:] == UNTOUCHED).all()
    assert (m["pcp"][:, :, :A] == UNTOUCHED).all() and (m["pcn"][:, :, :A] == UNTOUCHED).all()
    assert (m["pc"][:, :B, :A + D] != UNTOUCHED).any() and (m["pc"][:, B:] == UNTOUCHED).all()
    for in_max, e in ((0.3, 14), (37.5, 9)):
        m = RR.gather_model(obs, act, nobs, z, z, T, 1, 0, 8, 8, plane_mode=2, pa_ld=8, pc_ld=8, pa_next=4, pa_rows=8,
                            pc_rows=4, in_max=in_max)
        assert m["e"] == e and m["pa"].shape[0] == 2
        hw, lw = split2h(act, e)
        assert np.array_equal(m["pc"][0, :B, :A], hw) and np.array_equal(m["pc"][1, :B, :A], lw)


def test_small_models():
    counts, rows = RR.task_rows_model([2, 0, 2, 2, 0], 3, 2)
    assert counts.tolist() == [2, 0, 3] and rows.tolist() == [[1, 4], [-1, -1], [0, 2]]
    T, D, A, R = 2, 3, 2, 12
    obs, nobs = np.arange(6, dtype=f32).reshape(T, D), -np.arange(6, dtype=f32).reshape(T, D) - 10
    act, rew, done = np.full((T, A), 0.5, f32), np.array([100, -7], f32), np.array([50, 0], f32)
    rec, mn, mx, bm = RR.pack_commit_model(obs, nobs, act, rew, done, R, np.array([0.0, 0.0]), np.array([1.0, 1.0]), 2.0)
    assert rec.shape == (T, R) and (rec[:, 2 * D + A + 2:] == 0).all() and rec[1].tolist()[:7] == [3, 4, 5, 0.5, 0.5, -7, 0]
    assert mn.tolist() == [0, -7] and mx.tolist() == [100, 1] and bm == 15  # not the reward 100 or the done 50
    assert RR.pack_commit_model(obs, nobs, act, rew, done, R, mn, mx, 99.0)[3] == 99
    assert RR.absmax_model(np.array([1, -3, 2], f32), 0.5) == 3 and RR.absmax_model(np.array([1], f32), 4.0) == 4


def test_fill_model():
    cap, T_l, D, A, T_glob, tb = 2, 2, 9, 3, 3, 1
    store, bound, exact = RR.fill_model(cap, T_l, D, A, T_glob, tb, 5)
    R, F = RR.record_width(D, A), D - T_glob
    assert store.shape == (cap, T_l, R) and exact.sum() == R - 2 * F
    for t in range(T_l):
        oh = np.zeros(T_glob); oh[tb + t] = 1
        assert (store[:, t, F:D] == oh).all() and (store[:, t, D + A + 2 + F:2 * D + A + 2] == oh).all()
    assert (np.abs(store[..., D:D + A]) <= 1).all() and ((store[..., D + A] >= 0) & (store[..., D + A] < 10)).all()
    assert (bound[..., :F] >= 9 * 2.0 ** -23).all() and (bound[..., exact] == 0).all()
    assert (store[..., 2 * D + A + 2:] == 0).all()
