"""The reference values of one head-kernel case (tests/sac_head_cases.py) with the bar of every output element,
composed from the tolerance rule of tests/sac_head_ref.py: c 2^-24 S for the sums, the error a sum's bar
carries through the few float32 operations after it, and TAIL_FACTOR times the measured float32 spread for
the transcendental tails.  Nothing here looks at a kernel's output.  Shared by the GPU tests and by the CPU
tests that show what the bars reject and accept."""

from __future__ import annotations

import numpy as np

import sac_head_cases as C
import sac_head_ref as R

U, TF, LIBM = R.U, R.TAIL_FACTOR, R.LIBM_ULP
f32, f64 = np.float32, np.float64
GAMMA = 0.99


def tail_f32(out, eps):
    """The policy tail in float32 numpy from the float32-rounded head outputs: sigma, x, a, logpi."""
    A = out.shape[1] // 2
    o32, e32 = out.astype(f32), eps.astype(f32)
    mu32, ls32 = o32[:, :A], o32[:, A:]
    sg32 = np.exp(np.clip(ls32, f32(C.LS_MIN), f32(C.LS_MAX)))
    x32 = mu32 + sg32 * e32
    a32 = np.tanh(x32)
    sp32 = np.maximum(-2 * x32, 0) + np.log1p(np.exp(-np.abs(2 * x32)))
    lp32 = np.sum(f32(-0.5) * e32 * e32 - f32(R.HALF_LOG_2PI) - np.log(sg32) - f32(2) * (f32(R.LOG2) - x32 - sp32), axis=1,
                  dtype=f32)
    assert lp32.dtype == f32 and a32.dtype == f32 and x32.dtype == f32
    return sg32, x32, a32, lp32


def policy_expect(c, s):
    """Reference, bars (cache, a, logpi) and the measured float32 spread of row set s of a policy case."""
    A, W = c["A"], c["W"]
    r = R.policy_head(c["h"][s].astype(f64), c["Wh"].astype(f64), c["bh"].astype(f64), c["task"], c["eps"][s].astype(f64),
                      C.LS_MIN, C.LS_MAX)
    b_out = R.sum_bound(R.c_dot(W), r["S_out"])
    b_mu, b_ls = b_out[:, :A], b_out[:, A:]
    sg32, x32, a32, lp32 = tail_f32(r["out"], c["eps"][s])
    eps = np.abs(r["eps"])
    sc_x = np.abs(r["mu"]) + np.abs(r["sigma"] * r["eps"])
    spread = dict(sigma=np.max(np.abs(sg32 - r["sigma"]) / r["sigma"]), x=np.max(np.abs(x32 - r["x"]) / np.maximum(sc_x, 1e-30)),
                  a=np.max(np.abs(a32 - r["a"])), logpi=np.max(np.abs(lp32 - r["logpi"]) / r["S_logpi"]))
    b_sigma = r["sigma"] * (b_ls + TF * spread["sigma"])
    b_x = b_mu + eps * b_sigma + TF * spread["x"] * sc_x
    b_a = (1 - r["a"] ** 2 + 2 * b_x) * b_x + TF * spread["a"]  # tanh' = 1 - a^2, second order covered
    b_lp = np.sum(2 * b_x + b_ls, axis=1) + TF * spread["logpi"] * r["S_logpi"]  # |d logpi / dx| = |2 tanh x| <= 2
    bounds = dict(cache=np.concatenate([b_mu, b_ls, b_x, b_a, np.zeros_like(b_mu)], axis=1), a=b_a, logpi=b_lp)
    return r, bounds, spread


def critic_expect(c, mode, fused, clip, tw):
    """Reference outputs of critic_head in one mode and their bars; also q and its bar."""
    E, B, W = c["E"], c["B"], c["W"]
    d = {k: c[k].astype(f64) for k in ("h", "Wh", "bh", "th", "tWh", "tbh", "rew", "done", "logpi", "log_alpha", "y", "tw")}
    task = c["task"]
    q, Sq = R.critic_q(d["h"], d["Wh"], d["bh"], task)
    bq = R.sum_bound(R.c_dot(W), Sq)
    alpha, _ = R.row_alpha(task, c["task_begin"], d["log_alpha"], c["T_glob"])
    w = d["tw"] if tw else np.ones(B)
    inv = f64(f32(1.0 / (E * B) if mode == 1 else 1.0 / B))
    out, bnd = {}, {}

    def target(qq, bqq):  # five float32 operations after the min, expf in alpha
        y = R.td_target(qq, alpha, d["logpi"], d["rew"], d["done"], GAMMA, clip)
        live = (1 - d["done"]) * GAMMA
        Sy = np.abs(d["rew"]) + live * (np.abs(qq.min(0)) + np.abs(alpha * d["logpi"]))
        return y, live * bqq.max(0) + (5 + LIBM) * U * Sy

    if mode == 0:
        out["y_out"], bnd["y_out"] = target(q, bq)
        return out, bnd, q, bq
    if mode == 1:
        if fused:
            qt, Sqt = R.critic_q(d["th"], d["tWh"], d["tbh"], task)
            y, by = target(qt, R.sum_bound(R.c_dot(W), Sqt))
            out["y_out"], bnd["y_out"] = y, by
        else:
            y, by = d["y"], np.zeros(B)
        r = R.critic_loss(q, y, w, inv, clip)
        e1 = (bq + by[None]) + U * (np.abs(r["qc"]) + np.abs(y)[None])  # the error of qc - y
        out.update(dq=r["dq"], row_a=r["row_a"], row_b=r["row_b"])
        bnd["dq"] = 2 * w[None] * inv * r["dcl"] * e1 + 6 * U * np.abs(r["dq"])
        bnd["row_a"] = (w[None] * (2 * np.abs(r["diff"]) * e1 + e1 ** 2)).sum(0) + (E + 4) * U * r["row_a"]
        bnd["row_b"] = bq.sum(0) + E * U * np.abs(r["qc"]).sum(0)
        if clip:  # a q within its error of a bound (not exactly on it) would make the clip factor ambiguous
            near = (np.abs(np.abs(q) - 5000) <= bq) & (np.abs(q) != 5000)
            assert not near.any()
        return out, bnd, q, bq
    r = R.actor_loss(q, alpha, d["logpi"], w, inv)
    gaps = np.diff(np.sort(q, axis=0), axis=0) if E > 1 else np.ones((1, B))
    assert not ((gaps > 0) & (gaps <= 2 * bq.max(0))).any(), "a near-tie of the min: the tie pattern is ambiguous"
    out.update(dq=r["dq"], row_a=r["row_a"], alpha_w=r["alpha_w"])
    bnd["dq"] = 3 * U * np.abs(r["dq"])
    bnd["row_a"] = w * bq.max(0) + (4 + LIBM) * U * w * (np.abs(alpha * d["logpi"]) + np.abs(q.min(0)))
    bnd["alpha_w"] = (3 + LIBM) * U * np.abs(r["alpha_w"])
    return out, bnd, q, bq


def slice_sums(dz, task, T_l):
    """dbp[e][4 t + rs][w]: the column sums of dz over the rows j of task t's list with (j mod 16) div 4 == rs."""
    E, B, W = dz.shape
    out = np.zeros((E, 4 * T_l, W))
    for t in range(T_l):
        rows = np.flatnonzero(np.asarray(task) == t)
        for rs in range(4):
            out[:, 4 * t + rs] = dz[:, rows[(np.arange(len(rows)) % 16) // 4 == rs]].sum(1)
    return out


def backward_expect(c):
    """Reference outputs of the head backward (dz, db, dbp, dWh, dbh) and their bars."""
    hd, T_l, task = c["hd"], c["T_l"], c["task"]
    r = R.head_backward(c["h"].astype(f64), c["Wh"].astype(f64), c["dout"].astype(f64), task, T_l)
    n_t = R.task_lists(task, T_l)[0]
    b_dz = R.sum_bound(2 * hd, r["S_dz"])
    want = dict(dz=r["dz"], db=r["db"], dbp=slice_sums(r["dz"], task, T_l), dWh=r["dWh"], dbh=r["dbh"])
    cw = np.array([R.c_wgrad(n) for n in n_t]).reshape(1, T_l, 1, 1)
    cb = np.array([R.c_bgrad(n) for n in n_t]).reshape(1, T_l, 1)
    cs = np.repeat([-(-n // 16) + 3 for n in n_t], 4).reshape(1, 4 * T_l, 1)  # a slice's chain: c_colsum less the finish
    bnd = dict(dz=b_dz, db=b_dz.sum(1) + R.sum_bound(R.c_colsum(int(n_t.max()), T_l), r["S_db"]),
               dbp=slice_sums(b_dz, task, T_l) + R.sum_bound(cs, slice_sums(np.abs(r["dz"]), task, T_l)),
               dWh=R.sum_bound(cw, r["S_dWh"]), dbh=R.sum_bound(cb, r["S_dbh"]))
    return want, bnd, r


def action_grad_expect(c, a_data):
    """Reference outputs of action_grad (dout, and with a_data row_explore, row_loss) and their bars."""
    A, E, Wc = c["A"], c["E"], c["Wc"]
    d = {k: c[k].astype(f64) for k in ("dz1", "W0", "cache", "alpha_w", "a_data", "row_loss")}
    ls, a, eps = d["cache"][:, A:2 * A], d["cache"][:, 3 * A:4 * A], d["cache"][:, 4 * A:]
    glp = d["alpha_w"][:, None]
    r = R.action_grad(d["dz1"], d["W0"], d["cache"], d["alpha_w"], C.LS_MIN, C.LS_MAX, d["a_data"] if a_data else None,
                      f64(c["explore_scale"]), d["row_loss"])
    b_ga = R.sum_bound(R.c_agrad(Wc, E), r["S_ga"])
    bnd = {}
    if a_data:
        e_d = U * (np.abs(d["a_data"][:, :A]) + np.abs(a))  # the rounding of a_data - a
        b_ga = b_ga + f64(c["explore_scale"]) * (e_d + 2 * U * np.abs(r["ex_d"])) + U * np.abs(r["g_a"])
        bnd["row_explore"] = (2 * np.abs(r["ex_d"]) * e_d + e_d ** 2).sum(1) / A + (A + 8) * U * r["row_explore"]
        bnd["row_loss"] = bnd["row_explore"] + U * (np.abs(d["row_loss"]) + r["row_explore"])
    g_x = r["dout"][:, :A]
    sg = np.exp(np.clip(ls, C.LS_MIN, C.LS_MAX))
    b_gx = (1 - a * a) * b_ga + 6 * U * (np.abs(r["g_a"]) * (1 + a * a) + 2 * np.abs(glp * a))
    b_gls = R.clip_grad_factor(ls, C.LS_MIN, C.LS_MAX) * (np.abs(sg * eps) * b_gx
                                                         + (4 + LIBM) * U * (np.abs(g_x * sg * eps) + np.abs(glp)))
    bnd["dout"] = np.concatenate([b_gx, b_gls], axis=1)
    return r, bnd
