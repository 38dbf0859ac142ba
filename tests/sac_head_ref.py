"""Plain float64 statements of the SAC head kernels (mtrl_amd/csrc/heads.hip), one function per kernel, from
the formulas of oracle/mtsac.py (tanh_normal_sample, tanh_normal_backward, clip_grad_factor, min_grad and the
loss lines of update).  No tiling, no row lists beyond "the rows of task t", no float32.

Every function that sums returns, beside the value, S = the sum of the |terms| of each output element: the
tolerance rule below is stated on it.

The tolerance rule
------------------
U = 2^-24 is the unit roundoff of float32 (round to nearest).  A float32 sum of products whose longest chain of
additions has c links is within  c U S  of the exact sum (first order in U; each link rounds once, an fma link
included), plus c 2^-149 where results underflow gradually (a denormal gradient times a weight: the relative
model holds only in the normal range).  `sum_bound(c, S)` is that bar and `within(got, ref, bound)` the
element-wise test: every element, NaN never passes.  c comes from the kernel's documented order, never from
its output:

 * head dot product (rows_dot): a lane takes 4 fma per 256-column pass when W % 4 == 0, else one per 64-column
   pass; then 6 shuffle levels over the wave; then the bias: `c_dot(W)`.  The largest here, W = 516: 12 + 6 + 1
   = 19.
 * head data grad dz: hd products and hd additions per element: 2 hd.
 * its column sums: a wave adds every 16th row of a task, ceil(n / 16) links; 3 cross-wave links; colsum_finish
   adds the 4 T_l chunks in order: `c_colsum(n, T_l)`.
 * head weight grad: a wave adds every 4th row of the task, ceil(n / 4) links, one more for the product's own
   rounding, 3 cross-wave links: `c_wgrad(n)`; n = 257: 69.
 * head bias grad: ceil(n / 256) links per thread, then an 8-level tree: `c_bgrad(n)`.
 * action grad: the fma chain runs on through the E members, E times the dot product's lane links, then the 6
   shuffle levels: `c_agrad(Wc, E)`.
The derived c of the widest case of each kind is printed by tests/test_gpu_head_kernels.py.

The transcendental tails (expf, tanhf, logf, log1pf in sigma, a, logpi) have no such chain.  For them the GPU
tests measure, on their own inputs, how far a float32 numpy evaluation of the reference lies from the float64
one, relative to the element's scale (TAIL_SPREAD in the test module records it), and allow TAIL_FACTOR times
that: device libm and numpy's float32 routines are each good to an ulp or two but differ from each other, and
the logpi tail chains four of them per action dimension, so two correct evaluations can lie a few spreads
apart.  The short scalar tails (TD target, losses, dq, alpha) are bounded by their operation count times U,
with LIBM_ULP ulps for each libm call in them.
"""

from __future__ import annotations

import math

import numpy as np

LOG2 = math.log(2.0)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
U = 2.0 ** -24
TAIL_FACTOR = 4.0
LIBM_ULP = 4.0


# ------------------------------------------------------------------ the tolerance rule
def c_dot(W: int) -> int:
    lane = 4 * -(-W // 256) if W % 4 == 0 else -(-W // 64)
    return lane + 6 + 1


def c_colsum(n: int, T_l: int) -> int:
    return -(-n // 16) + 3 + 4 * T_l


def c_wgrad(n: int) -> int:
    return -(-n // 4) + 1 + 3


def c_bgrad(n: int) -> int:
    return -(-n // 256) + 8


def c_agrad(Wc: int, E: int) -> int:
    return E * (c_dot(Wc) - 7) + 6


TINY = 2.0 ** -149  # the spacing of float32's subnormals: a link whose result underflows rounds to that grid


def sum_bound(c, S):
    return c * (U * np.asarray(S, np.float64) + TINY)


def within(got, ref, bound) -> bool:
    """Every element of got within bound of ref (a NaN in got fails)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return bool(np.all(np.abs(got - ref) <= bound))


def worst(got, ref, bound) -> float:
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------ task lists
def task_lists(task, T_l):
    """counts[t] and the rows of task t in ascending order (numpy's stable lists)."""
    task = np.asarray(task)
    rows = [np.flatnonzero(task == t) for t in range(T_l)]
    return np.array([len(r) for r in rows]), rows


# ------------------------------------------------------------------ policy head
def head_out(h, Wh, bh, task):
    """out[b][o] = sum_w h[b][w] Wh[t_b][w][o] + bh[t_b][o], and its S."""
    prod = h[:, :, None] * Wh[task]
    return prod.sum(1) + bh[task], np.abs(prod).sum(1) + np.abs(bh[task])


def softplus(z):
    return np.logaddexp(z, 0.0)


def tanh_normal_sample(out, eps, ls_min, ls_max):
    """oracle.mtsac.tanh_normal_sample.  Returns mu, ls, sigma, x, a, logpi and S_logpi (the |terms| of logpi)."""
    A = out.shape[1] // 2
    mu, ls = out[:, :A], out[:, A:]
    sigma = np.exp(np.clip(ls, ls_min, ls_max))
    x = mu + sigma * eps
    a = np.tanh(x)
    sp = softplus(-2.0 * x)
    logpi = np.sum(-0.5 * eps * eps - HALF_LOG_2PI - np.log(sigma), axis=1) - np.sum(2.0 * (LOG2 - x - sp), axis=1)
    S = np.sum(0.5 * eps * eps + HALF_LOG_2PI + np.abs(np.log(sigma)) + 2.0 * (LOG2 + np.abs(x) + sp), axis=1)
    return dict(mu=mu, ls=ls, sigma=sigma, x=x, a=a, logpi=logpi, S_logpi=S)


def policy_head(h, Wh, bh, task, eps, ls_min, ls_max):
    out, S = head_out(h, Wh, bh, task)
    r = tanh_normal_sample(out, eps, ls_min, ls_max)
    r.update(out=out, S_out=S, eps=eps, cache=np.concatenate([r["mu"], r["ls"], r["x"], r["a"], eps], axis=1))
    return r


def clip_grad_factor(v, lo, hi):
    """d clip(v, lo, hi) / dv under jax: 1 inside, 0.5 at a bound, 0 beyond."""
    return ((v > lo) & (v < hi)).astype(np.float64) + 0.5 * ((v == lo) | (v == hi))


def tanh_normal_backward(ls, a, eps, g_a, g_logpi, ls_min, ls_max):
    """oracle.mtsac.tanh_normal_backward from the cached ls, a, eps: dout [B][2A] = (g_mu | g_ls)."""
    sigma = np.exp(np.clip(ls, ls_min, ls_max))
    g_x = g_a * (1.0 - a * a) + g_logpi[:, None] * 2.0 * a
    g_ls = (g_x * sigma * eps - g_logpi[:, None]) * clip_grad_factor(ls, ls_min, ls_max)
    return np.concatenate([g_x, g_ls], axis=1)


# ------------------------------------------------------------------ critic head
def critic_q(h, Wh, bh, task):
    """q[e][b] = sum_w h[e][b][w] Wh[e][t_b][w] + bh[e][t_b], and its S."""
    prod = h * Wh[:, task]
    return prod.sum(2) + bh[:, task], np.abs(prod).sum(2) + np.abs(bh[:, task])


def min_grad(q):
    """d min_e q_e / d q_e: ties share equally."""
    ind = (q == q.min(axis=0, keepdims=True)).astype(np.float64)
    return ind / ind.sum(axis=0, keepdims=True)


def td_target(q, alpha, logpi, rew, done, gamma, clip):
    y = rew + (1.0 - done) * gamma * (q.min(axis=0) - alpha * logpi)
    return np.clip(y, -5000.0, 5000.0) if clip else y


def critic_loss(q, y, w, inv_norm, clip):
    """The critic's loss lines: dq [E][B], row_a = sum_e w (qc - y)^2, row_b = sum_e qc."""
    qc = np.clip(q, -5000.0, 5000.0) if clip else q
    dcl = clip_grad_factor(q, -5000.0, 5000.0) if clip else np.ones_like(q)
    diff = qc - y[None]
    return dict(dq=w[None] * 2.0 * diff * inv_norm * dcl, row_a=(w[None] * diff * diff).sum(0), row_b=qc.sum(0), qc=qc,
                dcl=dcl, diff=diff)


def actor_loss(q, alpha, logpi, w, inv_norm):
    """The actor's: dq = -w inv_norm min_grad(q), row_a = w (alpha logpi - min q), alpha_w = w alpha inv_norm."""
    return dict(dq=-(w * inv_norm)[None] * min_grad(q), row_a=w * (alpha * logpi - q.min(axis=0)),
                alpha_w=w * alpha * inv_norm)


def row_alpha(task, task_begin, log_alpha, T_glob):
    """alpha[b] = exp(log_alpha[t]) and tw[b] = T softmax(-log_alpha)[t] (extract_task_weights)."""
    tg = task_begin + np.asarray(task)
    e = np.exp(-log_alpha - np.max(-log_alpha))
    return np.exp(log_alpha[tg]), (e / e.sum())[tg] * T_glob


# ------------------------------------------------------------------ head backward
def head_backward(h, Wh, dout, task, T_l):
    """h [E][B][W], Wh [E][T][W][hd], dout [E][B][hd]:
    dz = (dout . Wh[t_b]^T) (h > 0), db = its column sums, dWh[e][t] = sum over the rows of t of h (x) dout,
    dbh[e][t] = sum of dout; each with its S."""
    E, B, W = h.shape
    hd = dout.shape[2]
    prod = dout[:, :, None, :] * Wh[:, task]  # [E][B][W][hd]
    mask = h > 0
    dz, S_dz = prod.sum(3) * mask, np.abs(prod).sum(3) * mask
    dWh, S_dWh = np.zeros((E, T_l, W, hd)), np.zeros((E, T_l, W, hd))
    dbh, S_dbh = np.zeros((E, T_l, hd)), np.zeros((E, T_l, hd))
    for t in range(T_l):
        r = np.flatnonzero(np.asarray(task) == t)
        p = h[:, r, :, None] * dout[:, r, None, :]
        dWh[:, t], S_dWh[:, t] = p.sum(1), np.abs(p).sum(1)
        dbh[:, t], S_dbh[:, t] = dout[:, r].sum(1), np.abs(dout[:, r]).sum(1)
    return dict(dz=dz, S_dz=S_dz, db=dz.sum(1), S_db=np.abs(dz).sum(1), dWh=dWh, S_dWh=S_dWh, dbh=dbh, S_dbh=S_dbh)


def active_rows(dq):
    """Per member: n, the rows with dq != 0 in ascending order (-0.0 is inactive, a denormal active), slot."""
    E, B = dq.shape
    n, rows, slot = np.zeros(E, np.int64), -np.ones((E, B), np.int64), -np.ones((E, B), np.int64)
    for e in range(E):
        r = np.flatnonzero(dq[e] != 0)
        n[e] = len(r)
        rows[e, : len(r)] = r
        slot[e, r] = np.arange(len(r))
    return n, rows, slot


# ------------------------------------------------------------------ action grad
def action_grad(dz1, W0, cache, alpha_w, ls_min, ls_max, a_data=None, explore_scale=0.0, row_loss=None):
    """g_a[b][j] = sum_e sum_w dz1[e][b][w] W0[e][j][w] (the critic's grad at the action columns), plus the explore
    term's, then tanh_normal_backward with g_logpi = alpha_w.  cache [B][5A] = mu, ls, x, a, eps."""
    A = cache.shape[1] // 5
    prod = dz1[:, :, None, :] * W0[:, None, :A, :]  # [E][B][A][Wc]
    g_a, S_ga = prod.sum((0, 3)), np.abs(prod).sum((0, 3))
    ls, a, eps = cache[:, A:2 * A], cache[:, 3 * A:4 * A], cache[:, 4 * A:]
    out = dict(g_crit=g_a, S_ga=S_ga)
    if a_data is not None:
        d = a_data[:, :A] - a
        ex = (d * d).sum(1) / A
        g_a = g_a + explore_scale * d
        out.update(row_explore=ex, row_loss=row_loss - ex, ex_d=d)
    out.update(g_a=g_a, dout=tanh_normal_backward(ls, a, eps, g_a, alpha_w, ls_min, ls_max))
    return out
