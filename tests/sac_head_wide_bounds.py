"""Tolerance constants and reference bars of the wide head kernels (mtrl_amd/csrc/heads_wide.h, hd = 2A > 8),
the counterpart of c_dot / c_wgrad / c_bgrad / c_colsum / c_agrad in tests/sac_head_ref.py.  The rule is that
module's: a float32 sum whose longest chain of additions has c links lies within c 2^-24 S of the exact sum, S
the sum of the |terms|.  Every c below is read off the summation order heads_wide.h documents, never off a
kernel's output.  The wide kernels sum on the f32-input MFMA, bitwise a k-ordered fmaf chain with one rounding
per link -- so c is the length of the longest chain, plus the links of whatever follows it (for a chain split
over KS partial sums: the longest partial chain plus the KS - 1 links that add the partials).  Links that add
an exact zero (the padding of a chain to the instruction's k = 4, rows past a task's count) round nothing and
are not counted.

 * head dot product (wide_dot): KS = 4 partial chains, partial g over the 16-k blocks g, g + 4, ... (the longest,
   `chain_len(W)` links, is partial 0's), 3 links for ((P0 + P1) + P2) + P3, then the bias:
   `c_dot_wide(W)` = chain_len(W) + 3 + 1.
 * head data grad dz: one chain over the hd outputs: `c_dz_wide(hd)` = hd.
 * its column sums per (task, row slice rs): a 16-row tile is added as a 4-level butterfly, the tiles rt = rs,
   rs + 4, ... of the task in order: `c_slice_wide(n)` = 4 + ceil(ceil(n / 16) / 4); colsum_finish then adds the
   4 T_l slices in order: `c_colsum_wide(n, T_l)`.
 * head weight grad: one chain over the task's n rows: `c_wgrad_wide(n)` = n.
 * head bias grad: thread o adds the task's n rows in order: `c_bgrad_wide(n)` = n.
 * action grad: wide_dot's partial chains over Wc, each continued through the E members, then the 3 links:
   `c_agrad_wide(Wc, E)` = E chain_len(Wc) + 3.

These c are larger than the narrow kernels' (which split a sum over 64 lanes and pay 6 shuffle levels): a bar
here is the worst case of a long chain, not a fitted figure."""

from __future__ import annotations

import numpy as np

import sac_head_bounds as Bd
import sac_head_cases as C
import sac_head_ref as R

U, TF, LIBM = R.U, R.TAIL_FACTOR, R.LIBM_ULP
f32, f64 = np.float32, np.float64


KS = 4  # partial sums of one forward / action-grad output (WIDE_KS in heads_wide.h)


def chain_len(K: int) -> int:
    """The links of the longest partial chain over K: partial 0's blocks 0, 4, 8, ... of 16 k each."""
    return sum(min(16, K - k0) for k0 in range(0, K, 16 * KS))


def c_dot_wide(W: int) -> int:
    return chain_len(W) + (KS - 1) + 1


def c_dz_wide(hd: int) -> int:
    return hd


def c_slice_wide(n: int) -> int:
    return 4 + -(-(-(-n // 16)) // 4)


def c_colsum_wide(n: int, T_l: int) -> int:
    return c_slice_wide(n) + 4 * T_l


def c_wgrad_wide(n: int) -> int:
    return max(n, 1)


def c_bgrad_wide(n: int) -> int:
    return max(n, 1)


def c_agrad_wide(Wc: int, E: int) -> int:
    return E * chain_len(Wc) + (KS - 1)


# ------------------------------------------------------------------ the documented orders, in float32 numpy
def k_order(K: int, g: int):
    """The k of wide_dot's partial chain g, in order: its blocks k0 = 16 (g + 4 i); in a block s = 0..3, then
    kk = 0..3, k = k0 + 4 kk + s."""
    return [k0 + 4 * kk + s for k0 in range(16 * g, K, 16 * KS) for s in range(4) for kk in range(4)
            if k0 + 4 * kk + s < K]


def chain_f32(acc, a, b):
    """One fmaf link on float32 arrays (the product is exact in float64; the sum rounds once more on the way to
    float32, which can differ from a true fma in the last bit of rare cases -- it stays a float32 chain)."""
    return (acc.astype(f64) + a.astype(f64) * b.astype(f64)).astype(f32)


def dot_f32(Arows, Bmat, order=None, acc=None):
    """acc[r][o] += sum_k Arows[r][k] Bmat[k][o] as one float32 chain per output in the given k order."""
    acc = np.zeros((Arows.shape[0], Bmat.shape[1]), f32) if acc is None else acc
    for k in (range(Arows.shape[1]) if order is None else order):
        acc = chain_f32(acc, Arows[:, k, None], Bmat[None, k, :])
    return acc


def join_f32(parts):
    """((P0 + P1) + P2) + P3 in float32."""
    acc = parts[0]
    for p in parts[1:]:
        acc = (acc + p).astype(f32)
    return acc


def head_out_f32(h, Wh, bh, task):
    """The wide policy head's outputs in its own order, float32."""
    out = np.zeros((h.shape[0], Wh.shape[2]), f32)
    for t in np.unique(task):
        r = np.flatnonzero(task == t)
        out[r] = join_f32([dot_f32(h[r], Wh[t], k_order(h.shape[1], g)) for g in range(KS)]) + bh[t]
    return out


def backward_f32(h, Wh, dout, task, T_l):
    """The wide head backward in its own orders, float32: dz, dbp (slices), dWh, dbh for one member."""
    B, W = h.shape
    hd = dout.shape[1]
    dz = np.zeros((B, W), f32)
    dbp, dWh, dbh = np.zeros((4 * T_l, W), f32), np.zeros((T_l, W, hd), f32), np.zeros((T_l, hd), f32)
    for t in range(T_l):
        r = np.flatnonzero(np.asarray(task) == t)
        if not len(r):
            continue
        dz[r] = dot_f32(dout[r], np.ascontiguousarray(Wh[t].T)) * (h[r] > 0)
        dWh[t] = dot_f32(np.ascontiguousarray(h[r].T), dout[r])
        for j in range(len(r)):
            dbh[t] = dbh[t] + dout[r[j]]
        for rt in range(-(-len(r) // 16)):
            tile = np.zeros((16, W), f32)
            tile[: len(r[16 * rt:16 * rt + 16])] = dz[r[16 * rt:16 * rt + 16]]
            for step in (1, 2, 4, 8):  # the butterfly over the tile row index
                tile = tile + tile[np.arange(16) ^ step]
            dbp[4 * t + rt % 4] = dbp[4 * t + rt % 4] + tile[0]
    return dict(dz=dz, dbp=dbp, dWh=dWh, dbh=dbh)


def action_grad_f32(dz1, W0, A):
    """ga[b][j] in the wide action grad's order (each partial chain member after member), float32."""
    parts = [None] * KS
    for g in range(KS):
        for e in range(dz1.shape[0]):
            parts[g] = dot_f32(dz1[e], np.ascontiguousarray(W0[e, :A].T), k_order(dz1.shape[2], g), parts[g])
    return join_f32(parts)


# ------------------------------------------------------------------ references and bars
def policy_expect(c, s):
    """sac_head_bounds.policy_expect with the head outputs' bar from c_dot_wide; the tail rule unchanged."""
    A, W = c["A"], c["W"]
    r, _, spread = Bd.policy_expect(c, s)
    b_out = R.sum_bound(c_dot_wide(W), r["S_out"])
    b_mu, b_ls = b_out[:, :A], b_out[:, A:]
    eps = np.abs(r["eps"])
    sc_x = np.abs(r["mu"]) + np.abs(r["sigma"] * r["eps"])
    b_sigma = r["sigma"] * (b_ls + TF * spread["sigma"])
    b_x = b_mu + eps * b_sigma + TF * spread["x"] * sc_x
    b_a = (1 - r["a"] ** 2 + 2 * b_x) * b_x + TF * spread["a"]
    b_lp = np.sum(2 * b_x + b_ls, axis=1) + TF * spread["logpi"] * r["S_logpi"]
    bounds = dict(cache=np.concatenate([b_mu, b_ls, b_x, b_a, np.zeros_like(b_mu)], axis=1), a=b_a, logpi=b_lp,
                  out=b_out)
    return r, bounds, spread


def slice_sums(dz, task, T_l):
    """dbp[e][4 t + rs][w]: the column sums of dz over the rows j of task t's list with (j div 16) mod 4 == rs."""
    E, B, W = dz.shape
    out = np.zeros((E, 4 * T_l, W))
    for t in range(T_l):
        rows = np.flatnonzero(np.asarray(task) == t)
        for rs in range(4):
            out[:, 4 * t + rs] = dz[:, rows[(np.arange(len(rows)) // 16) % 4 == rs]].sum(1)
    return out


def backward_expect(c):
    """Reference outputs of the wide head backward (dz, db, dbp, dWh, dbh) and their bars."""
    hd, T_l, task = c["hd"], c["T_l"], c["task"]
    r = R.head_backward(c["h"].astype(f64), c["Wh"].astype(f64), c["dout"].astype(f64), task, T_l)
    n_t = R.task_lists(task, T_l)[0]
    b_dz = R.sum_bound(c_dz_wide(hd), r["S_dz"])
    want = dict(dz=r["dz"], db=r["db"], dbp=slice_sums(r["dz"], task, T_l), dWh=r["dWh"], dbh=r["dbh"])
    cw = np.array([c_wgrad_wide(n) for n in n_t]).reshape(1, T_l, 1, 1)
    cb = np.array([c_bgrad_wide(n) for n in n_t]).reshape(1, T_l, 1)
    cs = np.repeat([c_slice_wide(n) for n in n_t], 4).reshape(1, 4 * T_l, 1)
    bnd = dict(dz=b_dz, db=b_dz.sum(1) + R.sum_bound(c_colsum_wide(int(n_t.max()), T_l), r["S_db"]),
               dbp=slice_sums(b_dz, task, T_l) + R.sum_bound(cs, slice_sums(np.abs(r["dz"]), task, T_l)),
               dWh=R.sum_bound(cw, r["S_dWh"]), dbh=R.sum_bound(cb, r["S_dbh"]))
    return want, bnd, r


def action_grad_expect(c, a_data):
    """sac_head_bounds.action_grad_expect with the critic term's bar from c_agrad_wide."""
    A, E, Wc = c["A"], c["E"], c["Wc"]
    d = {k: c[k].astype(f64) for k in ("dz1", "W0", "cache", "alpha_w", "a_data", "row_loss")}
    ls, a, eps = d["cache"][:, A:2 * A], d["cache"][:, 3 * A:4 * A], d["cache"][:, 4 * A:]
    glp = d["alpha_w"][:, None]
    r = R.action_grad(d["dz1"], d["W0"], d["cache"], d["alpha_w"], C.LS_MIN, C.LS_MAX, d["a_data"] if a_data else None,
                      f64(c["explore_scale"]), d["row_loss"])
    b_ga = R.sum_bound(c_agrad_wide(Wc, E), r["S_ga"])
    bnd = {"ga": b_ga}
    if a_data:
        e_d = U * (np.abs(d["a_data"][:, :A]) + np.abs(a))
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
