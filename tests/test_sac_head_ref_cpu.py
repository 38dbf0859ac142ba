"""CPU checks of the head-kernel reference (tests/sac_head_ref.py) and of its tolerance rule:
 * every backward function against central finite differences of its forward, in float64;
 * the composed functions against the intermediate values of oracle.mtsac.update at a small config with
   action_dim 3 and num_critics 3;
 * the bars of tests/sac_head_bounds.py reject a set of seeded errors applied to the reference output, and
   accept a float32 numpy evaluation of the reference in another summation order."""

from __future__ import annotations

import numpy as np
import pytest

import sac_head_bounds as Bd
import sac_head_cases as C
import sac_head_ref as R
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

f32, f64 = np.float32, np.float64


def _fd(f, x, h=1e-6):
    """Central differences of the scalar f at x, element by element."""
    g = np.zeros_like(x)
    for i in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


# ------------------------------------------------------------------ finite differences
def test_clip_grad_factor_is_the_central_difference_of_clip():
    v = np.array([-3.0, -2.0, -1.0, 0.5, 1.0, 1.5])
    fd = _fd(lambda x: np.clip(x, C.LS_MIN, C.LS_MAX).sum(), v)
    np.testing.assert_allclose(R.clip_grad_factor(v, C.LS_MIN, C.LS_MAX), fd, atol=1e-9)
    assert R.clip_grad_factor(v, C.LS_MIN, C.LS_MAX).tolist() == [0, 0.5, 1, 1, 0.5, 0]


def test_min_grad_matches_finite_differences_and_shares_ties():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((4, 6))
    np.testing.assert_allclose(R.min_grad(q), _fd(lambda x: x.min(0).sum(), q), atol=1e-8)
    q[[0, 2, 3], 1] = q[:, 1].min() - 1.0  # a three-way tie: a third each
    assert R.min_grad(q)[:, 1].tolist() == [1 / 3, 0, 1 / 3, 1 / 3]


def test_tanh_normal_backward_matches_finite_differences():
    rng = np.random.default_rng(1)
    B, A = 7, 3
    out = rng.standard_normal((B, 2 * A))
    out[0, A:] = C.LS_MAX + 0.3  # beyond the bounds: no gradient through the log-std
    out[1, A:] = C.LS_MIN - 0.3
    eps = rng.standard_normal((B, A))
    g_a, g_lp = rng.standard_normal((B, A)), rng.standard_normal(B)

    def f(o):
        r = R.tanh_normal_sample(o, eps, C.LS_MIN, C.LS_MAX)
        return (r["a"] * g_a).sum() + (r["logpi"] * g_lp).sum()

    r = R.tanh_normal_sample(out, eps, C.LS_MIN, C.LS_MAX)
    got = R.tanh_normal_backward(r["ls"], r["a"], eps, g_a, g_lp, C.LS_MIN, C.LS_MAX)
    np.testing.assert_allclose(got, _fd(f, out), rtol=1e-6, atol=1e-7)
    assert (got[:2, A:] == 0).all()


def test_head_backward_matches_finite_differences():
    rng = np.random.default_rng(2)
    E, B, W, hd, T_l = 2, 9, 5, 3, 3
    task = rng.integers(0, T_l - 1, B)  # the last task stays empty
    z = rng.standard_normal((E, B, W))  # pre-activations, away from 0
    z[np.abs(z) < 0.05] = 0.5
    Wh, bh = rng.standard_normal((E, T_l, W, hd)), rng.standard_normal((E, T_l, hd))
    dout = rng.standard_normal((E, B, hd))

    def loss(z_, Wh_, bh_):
        h = np.maximum(z_, 0)
        return sum((R.head_out(h[e], Wh_[e], bh_[e], task)[0] * dout[e]).sum() for e in range(E))

    r = R.head_backward(np.maximum(z, 0), Wh, dout, task, T_l)
    np.testing.assert_allclose(r["dz"], _fd(lambda x: loss(x, Wh, bh), z), atol=1e-7)
    np.testing.assert_allclose(r["dWh"], _fd(lambda x: loss(z, x, bh), Wh), atol=1e-7)
    np.testing.assert_allclose(r["dbh"], _fd(lambda x: loss(z, Wh, x), bh), atol=1e-7)
    np.testing.assert_allclose(r["db"], r["dz"].sum(1))
    assert (r["dWh"][:, T_l - 1] == 0).all() and (r["dbh"][:, T_l - 1] == 0).all()
    # hd = 1 is the critic's head: critic_q is head_out per member
    q, _ = R.critic_q(np.maximum(z, 0), Wh[..., 0], bh[..., 0], task)
    np.testing.assert_allclose(q[1], R.head_out(np.maximum(z[1], 0), Wh[1, :, :, :1], bh[1, :, :1], task)[0][:, 0])


@pytest.mark.parametrize("clip", [False, True])
def test_loss_gradients_match_finite_differences(clip):
    rng = np.random.default_rng(3)
    E, B = 3, 8
    q = rng.standard_normal((E, B)) * 3
    if clip:  # rows 0 and 1 near the bounds (targets there too, so the squares stay small enough for differences)
        q[:, 0], q[:, 1] = 4998.0 + q[:, 0] / 3, -4998.0 + q[:, 1] / 3
        q[0, 0], q[1, 1] = 5300.0, -5100.0  # beyond the bounds: no gradient
    y, w = rng.standard_normal(B), rng.uniform(0.5, 1.5, B)
    if clip:
        y[0], y[1] = 4999.0, -4999.5
    alpha, logpi = rng.uniform(0.5, 2, B), rng.standard_normal(B)
    inv = 1.0 / (E * B)
    r = R.critic_loss(q, y, w, inv, clip)
    np.testing.assert_allclose(r["dq"], _fd(lambda x: inv * R.critic_loss(x, y, w, inv, clip)["row_a"].sum(), q, 1e-5),
                               rtol=1e-6, atol=1e-8)
    if clip:
        assert r["dq"][0, 0] == 0 and r["dq"][1, 1] == 0
    a = R.actor_loss(q, alpha, logpi, w, 1.0 / B)
    np.testing.assert_allclose(a["dq"], _fd(lambda x: R.actor_loss(x, alpha, logpi, w, 1.0)["row_a"].sum() / B, q, 1e-5),
                               rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(a["alpha_w"], _fd(lambda x: R.actor_loss(q, alpha, x, w, 1.0)["row_a"].sum() / B, logpi),
                               rtol=1e-6, atol=1e-8)
    # the TD target: gamma (1 - done) of the min's gradient
    done = (np.arange(B) % 2).astype(f64)
    gy = _fd(lambda x: R.td_target(x, alpha, logpi, y, done, 0.99, False).sum(), q)
    np.testing.assert_allclose(gy, 0.99 * (1 - done)[None] * R.min_grad(q), atol=2e-6)  # differences of values ~5000


def test_action_grad_matches_finite_differences():
    """The whole chain behind dout: the head outputs (mu | ls) -> a, logpi -> a critic linear in a, the
    temperature term alpha_w logpi and the explore term -(1/n) mean_j (a_data - a)^2."""
    rng = np.random.default_rng(4)
    E, B, A, Wc = 2, 5, 3, 6
    out = rng.standard_normal((B, 2 * A))
    out[0, A] = C.LS_MAX + 0.2
    eps = rng.standard_normal((B, A))
    dz1, W0 = rng.standard_normal((E, B, Wc)), rng.standard_normal((E, A + 4, Wc))
    alpha_w, a_data = rng.uniform(0, 1, B), rng.uniform(-1, 1, (B, A + 2))
    scale = 2.0 / (B * A)

    def f(o, explore):
        r = R.tanh_normal_sample(o, eps, C.LS_MIN, C.LS_MAX)
        crit = sum(((r["a"] @ W0[e, :A]) * dz1[e]).sum() for e in range(E))  # the action columns of layer 0
        ex = ((a_data[:, :A] - r["a"]) ** 2).sum(1) / A
        return crit + (alpha_w * r["logpi"]).sum() - (ex.sum() / B if explore else 0.0)

    r = R.tanh_normal_sample(out, eps, C.LS_MIN, C.LS_MAX)
    cache = np.concatenate([r["mu"], r["ls"], r["x"], r["a"], eps], axis=1)
    for explore in (False, True):
        g = R.action_grad(dz1, W0, cache, alpha_w, C.LS_MIN, C.LS_MAX, a_data if explore else None, scale, np.zeros(B))
        np.testing.assert_allclose(g["dout"], _fd(lambda o: f(o, explore), out), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(g["row_loss"], -g["row_explore"])
    assert g["dout"][0, A] == 0


# ------------------------------------------------------------------ against oracle.mtsac.update
def test_composed_functions_reproduce_the_oracle_update():
    T, W, n, A, Cn = 3, 16, 4, 3, 3
    B = n * T
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A, num_critics=Cn,
                          clip=True, use_task_weights=True)
    st = om.initialize(cfg, seed=7)
    st.log_alpha = np.array([0.3, -0.2, 0.1])
    obs, act, nobs, done, rew = synthetic_batch(T, B, action_dim=A, seed=1)
    en, ec = synthetic_eps(B, action_dim=A, seed=2)
    new, _, it = om.update(cfg, st, (obs, act, nobs, done, rew), en, ec, return_internals=True)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc, pt = om.unflatten(st.actor, ash), om.unflatten(st.critic, csh), om.unflatten(st.critic_target, csh)
    pc_new = om.unflatten(new.critic, csh)
    task = om.task_index(obs, T)
    lo, hi = cfg.log_std_min, cfg.log_std_max
    alpha, tw = R.row_alpha(task, 0, st.log_alpha, T)
    np.testing.assert_allclose(alpha, it["alpha_rows"][:, 0], rtol=1e-14)

    def top(p, x, depth):
        return om.mh_forward(p, x, depth, T)[1]

    def critic_tops(p, x):
        hs = [top(om.ens_slice(p, k), x, cfg.critic_depth) for k in range(Cn)]
        return hs, np.stack([h[-1] for h in hs])

    # critic step: a' ~ pi(.|s'), the target, the loss lines, the head backward
    pn = R.policy_head(top(pa, nobs, cfg.actor_depth)[-1], pa["head_W"], pa["head_b"], task, en, lo, hi)
    np.testing.assert_allclose(pn["a"], it["a_next"], rtol=1e-12)
    np.testing.assert_allclose(pn["logpi"], it["logpi_next"], rtol=1e-12)
    _, ht = critic_tops(pt, np.concatenate([pn["a"], nobs], axis=1))
    qt, _ = R.critic_q(ht, pt["head_W"][..., 0], pt["head_b"][..., 0], task)
    np.testing.assert_allclose(qt, it["q_target"][..., 0], rtol=1e-12)
    y = R.td_target(qt, alpha, pn["logpi"], rew[:, 0], done[:, 0], cfg.gamma, True)
    np.testing.assert_allclose(y, it["y"][:, 0], rtol=1e-12)
    _, hc = critic_tops(pc, np.concatenate([act, obs], axis=1))
    q, _ = R.critic_q(hc, pc["head_W"][..., 0], pc["head_b"][..., 0], task)
    np.testing.assert_allclose(q, it["q"][..., 0], rtol=1e-12)
    cl = R.critic_loss(q, y, tw, 1.0 / (Cn * B), True)
    hb = R.head_backward(hc, pc["head_W"], cl["dq"][..., None], task, T)
    gc = om.unflatten(it["critic_grad"], csh)
    np.testing.assert_allclose(hb["dWh"], gc["head_W"], rtol=1e-10, atol=1e-16)
    np.testing.assert_allclose(hb["dbh"], gc["head_b"], rtol=1e-10, atol=1e-16)
    np.testing.assert_allclose(hb["db"], gc[f"b{cfg.critic_depth - 1}"], rtol=1e-10, atol=1e-16)

    # actor step: a ~ pi(.|s), the actor loss through the updated critic, the action grad, the head backward
    ha = top(pa, obs, cfg.actor_depth)[-1]
    pcur = R.policy_head(ha, pa["head_W"], pa["head_b"], task, ec, lo, hi)
    np.testing.assert_allclose(pcur["a"], it["a_cur"], rtol=1e-12)
    np.testing.assert_allclose(pcur["logpi"], it["logpi_cur"], rtol=1e-12)
    hs_pi, hpi = critic_tops(pc_new, np.concatenate([pcur["a"], obs], axis=1))
    qpi, _ = R.critic_q(hpi, pc_new["head_W"][..., 0], pc_new["head_b"][..., 0], task)
    np.testing.assert_allclose(qpi, it["q_pi"][..., 0], rtol=1e-12)
    al = R.actor_loss(qpi, alpha, pcur["logpi"], tw, 1.0 / B)
    dz = R.head_backward(hpi, pc_new["head_W"], al["dq"][..., None], task, T)["dz"]  # at the top layer's pre-activation
    for i in reversed(range(1, cfg.critic_depth)):  # down the trunk to layer 0's
        dz = np.stack([(dz[k] @ pc_new[f"W{i}"][k].T) * (hs_pi[k][i] > 0) for k in range(Cn)])
    ag = R.action_grad(dz, pc_new["W0"], pcur["cache"], al["alpha_w"], lo, hi)
    np.testing.assert_allclose(ag["g_a"], it["g_a"], rtol=1e-9, atol=1e-16)
    hba = R.head_backward(ha[None], pa["head_W"][None], ag["dout"][None], task, T)
    ga = om.unflatten(it["actor_grad"], ash)
    np.testing.assert_allclose(hba["dWh"][0], ga["head_W"], rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(hba["dbh"][0], ga["head_b"], rtol=1e-9, atol=1e-16)
    np.testing.assert_allclose(hba["db"][0], ga[f"b{cfg.actor_depth - 1}"], rtol=1e-9, atol=1e-16)


# ------------------------------------------------------------------ what the bars reject and accept
COUNTS = (3, 4, 0, 65, 17)  # an empty task, 17 = one row into a second 16-row group, 65 into a fifth


def _f32_sum(x, axis):
    """A float32 sum in another order than any kernel's: reversed, numpy's pairwise tree."""
    x = np.flip(np.asarray(x, f32), axis)
    out = x.sum(axis=axis, dtype=f32)
    assert out.dtype == f32
    return out


def test_bars_reject_seeded_errors_in_the_head_backward():
    c = C.backward_case(4, 1, 260, COUNTS)
    want, bnd, r = Bd.backward_expect(c)
    task, T_l = c["task"], c["T_l"]
    h, dout = c["h"].astype(f64), c["dout"].astype(f64)
    assert all(R.within(want[k], want[k], bnd[k]) for k in want)
    # one row dropped from a task's weight-grad sum (a row whose gradient and activation are not all zero)
    rows = np.flatnonzero(task == 3)
    b = next(int(b) for b in rows if np.abs(dout[0, b]).max() > 0.1 and h[0, b].max() > 0.1)
    bad = want["dWh"].copy()
    bad[0, 3] -= h[0, b][:, None] * dout[0, b][None, :]
    assert not R.within(bad, want["dWh"], bnd["dWh"])
    bad = want["dbh"].copy()
    bad[0, 3] -= dout[0, b]
    assert not R.within(bad, want["dbh"], bnd["dbh"])
    # the last row of a partial row group skipped: task 4 has 17 rows, the 17th alone in its second group of 16
    last = int(np.flatnonzero(task == 4)[16])
    assert np.abs(r["dz"][0, last]).max() > 0.1, "the skipped row must carry a gradient"
    bad = want["db"].copy() - r["dz"][:, last]
    assert not R.within(bad, want["db"], bnd["db"])
    bad = want["dz"].copy()
    bad[0, last] = 0
    assert not R.within(bad, want["dz"], bnd["dz"])
    # one element off by 2^-10 relative, where the element is not a cancellation
    for k in ("dz", "dWh", "dbh", "db"):
        i = np.unravel_index(np.argmax(np.abs(want[k]) / np.maximum(bnd[k], 1e-300)), want[k].shape)
        bad = want[k].copy()
        bad[i] *= 1 + 2.0 ** -10
        assert not R.within(bad, want[k], bnd[k]), k


def test_bars_reject_seeded_errors_in_the_policy_and_critic_heads():
    c = C.policy_case(2, 260, COUNTS)
    A = c["A"]
    r, bnd, _ = Bd.policy_expect(c, 0)
    assert R.within(r["cache"], r["cache"], bnd["cache"]) and R.within(r["logpi"], r["logpi"], bnd["logpi"])
    # mu and log-std columns swapped
    sw = R.tanh_normal_sample(np.concatenate([r["out"][:, A:], r["out"][:, :A]], axis=1), r["eps"], C.LS_MIN, C.LS_MAX)
    assert not R.within(sw["a"], r["a"], bnd["a"]) and not R.within(sw["logpi"], r["logpi"], bnd["logpi"])
    # one element off by 2^-10 relative
    for k, ref in (("a", r["a"]), ("logpi", r["logpi"]), ("cache", r["cache"])):
        i = np.unravel_index(np.argmax(np.abs(ref) / np.maximum(bnd[k], 1e-300)), ref.shape)
        bad = ref.copy()
        bad[i] *= 1 + 2.0 ** -10
        assert not R.within(bad, ref, bnd[k]), k
    # a clip tie factor of 1 instead of 0.5, on the log-std (action grad) ...
    g = C.action_grad_case(2, 2, 260, 17)
    ra, ba = Bd.action_grad_expect(g, False)
    ls = g["cache"][:, 2:4].astype(f64)
    tie = (ls == C.LS_MIN) | (ls == C.LS_MAX)
    assert tie.any()
    bad = ra["dout"].copy()
    bad[:, 2:][tie] *= 2
    assert not R.within(bad, ra["dout"], ba["dout"])
    # ... and on q at +-5000 (critic loss with clip)
    cc = C.critic_case(4, 260, COUNTS)
    want, cb, q, _ = Bd.critic_expect(cc, 1, False, True, False)
    assert (np.abs(q) == 5000).any()
    bad = want["dq"].copy()
    bad[np.abs(q) == 5000] *= 2
    assert not R.within(bad, want["dq"], cb["dq"])
    # a min tie credited to one member instead of shared
    want, cb, q, _ = Bd.critic_expect(cc, 2, False, False, False)
    cnt = (q == q.min(0)).sum(0)
    assert {2, 3, 4} <= set(cnt.tolist())
    for n in (2, 3, 4):
        b = int(np.flatnonzero(cnt == n)[0])
        bad = want["dq"].copy()
        first = int(np.argmin(q[:, b]))
        bad[:, b] = 0
        bad[first, b] = want["dq"][:, b].sum()
        assert not R.within(bad, want["dq"], cb["dq"]), n
    # done ignored in the TD target
    want, cb, q, _ = Bd.critic_expect(cc, 0, False, False, False)
    d = {k: cc[k].astype(f64) for k in ("logpi", "rew", "done", "log_alpha")}
    alpha, _ = R.row_alpha(cc["task"], cc["task_begin"], d["log_alpha"], cc["T_glob"])
    bad = R.td_target(q, alpha, d["logpi"], d["rew"], np.zeros_like(d["done"]), Bd.GAMMA, False)
    assert (d["done"] == 1).any() and not R.within(bad, want["y_out"], cb["y_out"])


def test_bars_accept_a_float32_evaluation_in_another_order():
    # head backward: float32 products, summed reversed and pairwise
    c = C.backward_case(4, 1, 260, COUNTS)
    want, bnd, _ = Bd.backward_expect(c)
    task, T_l, h, Wh, dout = c["task"], c["T_l"], c["h"], c["Wh"], c["dout"]
    dz = _f32_sum(dout[:, :, None, :] * Wh[:, task], 3) * (h > 0)
    assert R.within(dz, want["dz"], bnd["dz"])
    assert R.within(_f32_sum(dz, 1), want["db"], bnd["db"])
    for t in range(T_l):
        rows = np.flatnonzero(task == t)
        assert R.within(_f32_sum(h[:, rows, :, None] * dout[:, rows, None, :], 1), want["dWh"][:, t], bnd["dWh"][:, t])
        assert R.within(_f32_sum(dout[:, rows], 1), want["dbh"][:, t], bnd["dbh"][:, t])
    # policy head: float32 dot products in that order, then the float32 tail
    p = C.policy_case(3, 516, COUNTS)
    r, pb, _ = Bd.policy_expect(p, 0)
    out = _f32_sum(p["h"][0][:, :, None] * p["Wh"][p["task"]], 1) + p["bh"][p["task"]]
    assert out.dtype == f32
    sg, x, a, lp = Bd.tail_f32(out, p["eps"][0])
    A = p["A"]
    cache = np.concatenate([out[:, :A], out[:, A:], x, a, p["eps"][0]], axis=1)
    assert R.within(cache, r["cache"], pb["cache"]) and R.within(a, r["a"], pb["a"]) and R.within(lp, r["logpi"], pb["logpi"])
    # critic head, critic mode with the fused target and clip: float32 throughout
    cc = C.critic_case(3, 252, COUNTS)
    want, cb, _, _ = Bd.critic_expect(cc, 1, True, True, True)
    t = cc["task"]
    q = _f32_sum(cc["h"] * cc["Wh"][:, t], 2) + cc["bh"][:, t]
    qt = _f32_sum(cc["th"] * cc["tWh"][:, t], 2) + cc["tbh"][:, t]
    alpha = np.exp(cc["log_alpha"][cc["task_begin"] + t])
    y = cc["rew"] + (f32(1) - cc["done"]) * f32(Bd.GAMMA) * (qt.min(0) - alpha * cc["logpi"])
    y = np.clip(y, f32(-5000), f32(5000))
    qc = np.clip(q, f32(-5000), f32(5000))
    inv = f32(1.0 / (cc["E"] * cc["B"]))
    dq = cc["tw"][None] * f32(2) * (qc - y[None]) * inv * R.clip_grad_factor(q, -5000.0, 5000.0).astype(f32)
    assert dq.dtype == f32 and y.dtype == f32
    assert R.within(y, want["y_out"], cb["y_out"]) and R.within(dq, want["dq"], cb["dq"])
    assert R.within((cc["tw"][None] * (qc - y[None]) ** 2).sum(0, dtype=f32), want["row_a"], cb["row_a"])
    assert R.within(qc.sum(0, dtype=f32), want["row_b"], cb["row_b"])
    # action grad
    g = C.action_grad_case(3, 3, 130, 65)
    ra, ab = Bd.action_grad_expect(g, True)
    A = g["A"]
    ga = _f32_sum(_f32_sum(g["dz1"][:, :, None, :] * g["W0"][:, None, :A, :], 3), 0)
    ls, a, eps = g["cache"][:, A:2 * A], g["cache"][:, 3 * A:4 * A], g["cache"][:, 4 * A:]
    d = g["a_data"][:, :A] - a
    ga = ga + g["explore_scale"] * d
    glp = g["alpha_w"][:, None]
    gx = ga * (f32(1) - a * a) + glp * f32(2) * a
    gls = (gx * np.exp(np.clip(ls, f32(C.LS_MIN), f32(C.LS_MAX))) * eps - glp) * R.clip_grad_factor(ls, C.LS_MIN, C.LS_MAX).astype(f32)
    dout = np.concatenate([gx, gls], axis=1)
    assert dout.dtype == f32 and R.within(dout, ra["dout"], ab["dout"])
    ex = (d * d).sum(1, dtype=f32) / f32(A)
    assert R.within(ex, ra["row_explore"], ab["row_explore"]) and R.within(g["row_loss"] - ex, ra["row_loss"], ab["row_loss"])
