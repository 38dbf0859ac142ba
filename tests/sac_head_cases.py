"""Inputs of the SAC head kernel tests (tests/test_gpu_head_kernels.py, tests/test_sac_head_ref_cpu.py): float32
arrays drawn once per case, with the edge values placed on purpose.

Exact edge values.  Head biases are multiples of 1/64.  A special row's activation is one-hot, h = e_k, and
the head kernel's row k of its task is set to target - bias (exact in float32), so the head output of that
row is `target` exactly, on the device (an fma chain over one non-zero term) and in float64 alike.  Column 3
carries the large targets (tanh saturation, q = +-5000) and is zero in every ordinary row -- a dead ReLU unit
-- so the ordinary rows keep ordinary magnitudes.  Special row j < 4 of a task is that task's j-th row, so a
task with at least four rows holds all four."""

from __future__ import annotations

import functools

import numpy as np

LS_MIN, LS_MAX = -2.0, 1.0
f32 = np.float32


def tasks(counts, seed):
    """task[B] with counts[t] rows of task t, interleaved (round-robin with a seeded shuffle, never blocked)."""
    rng = np.random.default_rng(seed)
    t = np.concatenate([np.full(c, i, np.int32) for i, c in enumerate(counts)])
    t = t[rng.permutation(len(t))]
    if sum(c > 0 for c in counts) > 1 and not np.any(np.diff(t) < 0):
        t = np.roll(t, 1)  # the shuffle left them sorted: the last task's row goes first
    return t


def _grid(rng, *shape):
    return (rng.integers(-64, 65, shape) / 64.0).astype(f32)


def _special_rows(task, T_l):
    """{(t, j): row} for the first four rows j of every task."""
    return {(t, j): int(r) for t in range(T_l) for j, r in enumerate(np.flatnonzero(task == t)[:4])}


def _activations(rng, B, W):
    h = np.maximum(rng.standard_normal((B, W)), 0).astype(f32)
    h[:, 3] = 0
    return h


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def policy_case(A, W, counts, seed=0):
    """Two row sets (h, eps) over one task list for the actor head, hd = 2A.  Special rows per task: j = 0 the
    log-stds at a bound (max for even action dimensions, min for odd), j = 1 the other way round, j = 2 beyond
    the bounds, j = 3 the means at +-12 (tanh saturates in float32).  eps holds 0 and +-4."""
    T_l, B, hd = len(counts), sum(counts), 2 * A
    rng = np.random.default_rng(1000 * A + W + 7 * B + seed)
    task = tasks(counts, seed + W)
    Wh = (rng.standard_normal((T_l, W, hd)) / np.sqrt(W)).astype(f32)
    bh = _grid(rng, T_l, hd)
    tgt = np.zeros((4, hd))
    for j in range(A):
        tgt[0, A + j], tgt[1, A + j] = (LS_MAX, LS_MIN) if j % 2 == 0 else (LS_MIN, LS_MAX)
        tgt[2, A + j] = LS_MAX + 0.5 if j % 2 == 0 else LS_MIN - 1.0
        tgt[0, j], tgt[1, j], tgt[2, j] = 0.25 * j, -0.5, 0.125
        tgt[3, j], tgt[3, A + j] = (12.0 if j % 2 == 0 else -12.0), -0.75
    for t in range(T_l):
        Wh[t, :4] = (tgt - bh[t].astype(np.float64)).astype(f32)
    hs, es = [], []
    for s in range(2):
        h = _activations(rng, B, W)
        eps = rng.standard_normal((B, A)).astype(f32)
        for (t, j), r in _special_rows(task, T_l).items():
            h[r] = 0
            h[r, j] = 1
        eps.flat[s::7] = 0.0
        eps.flat[3 + s::11] = 4.0
        eps.flat[5 + s::13] = -4.0
        hs.append(h)
        es.append(eps)
    return _ro(dict(A=A, W=W, T_l=T_l, B=B, hd=hd, task=task, Wh=Wh, bh=bh, h=np.stack(hs), eps=np.stack(es),
                    special=_special_rows(task, T_l)))


@functools.lru_cache(maxsize=None)
def critic_case(E, W, counts, seed=0):
    """Critic and target-critic head inputs, hd = 1.  Special rows per task: j = 0, 1, 2 a tie of 2, 3, 4 members
    for the min (as many as E allows; the others larger), j = 3 q at +5000 (even members) / -5000 (odd) exactly;
    the row after them 1.5 there, so that q lies beyond the bound.  done holds 0 and 1."""
    T_l, B = len(counts), sum(counts)
    rng = np.random.default_rng(2000 * E + W + 7 * B + seed)
    task = tasks(counts, seed + W + 1)
    out = dict(E=E, W=W, T_l=T_l, B=B, task=task, special=_special_rows(task, T_l))
    sp = out["special"]
    beyond = {t: int(r[4]) for t in range(T_l) if len(r := np.flatnonzero(task == t)) > 4}
    tgt = np.zeros((E, 4))
    for e in range(E):
        for j in range(3):
            tgt[e, j] = -0.5 if e < j + 2 else 0.25 * (e + 1)
        tgt[e, 3] = 5000.0 if e % 2 == 0 else -5000.0
    for name in ("", "t"):
        Wh = (rng.standard_normal((E, T_l, W)) / np.sqrt(W)).astype(f32)
        bh = _grid(rng, E, T_l)
        for t in range(T_l):
            Wh[:, t, :4] = (tgt - bh[:, t, None].astype(np.float64)).astype(f32)
        h = np.stack([_activations(rng, B, W) for _ in range(E)])
        for (t, j), r in sp.items():
            h[:, r] = 0
            h[:, r, j] = 1
        for t, r in beyond.items():
            h[:, r, 3] = 1.5
        out.update({name + "Wh": Wh, name + "bh": bh, name + "h": h})
    out["beyond"] = beyond
    out["rew"] = rng.uniform(0, 10, B).astype(f32)
    out["done"] = (np.arange(B) % 3 == 1).astype(f32)
    out["logpi"] = rng.standard_normal(B).astype(f32) * 3
    out["y"] = rng.standard_normal(B).astype(f32) * 5
    out["tw"] = rng.uniform(0.5, 1.5, B).astype(f32)
    out["T_glob"], out["task_begin"] = T_l + 3, 2
    out["log_alpha"] = rng.uniform(-1, 1, T_l + 3).astype(f32)
    return _ro(out)


@functools.lru_cache(maxsize=None)
def backward_case(hd, E, W, counts, seed=0):
    """Head backward inputs: h with ReLU zeros (and -0.0, which masks too), dout with zero rows; for hd = 1 dout is
    a dq whose zeros (of both signs) and one denormal exercise active_rows."""
    T_l, B = len(counts), sum(counts)
    rng = np.random.default_rng(3000 * hd + 100 * E + W + 7 * B + seed)
    task = tasks(counts, seed + W + 2)
    h = np.maximum(rng.standard_normal((E, B, W)), 0).astype(f32)
    h.reshape(-1)[5::17] = -0.0
    Wh = (rng.standard_normal((E, T_l, W, hd)) / np.sqrt(W)).astype(f32)
    dout = rng.standard_normal((E, B, hd)).astype(f32)
    off = rng.uniform(size=(E, B)) < 0.4
    dout[off] = 0.0
    dout[:, 1::9] *= f32(-0.0) if hd == 1 else f32(1.0)
    if hd == 1 and B > 2:
        dout[0, 2, 0] = f32(1e-40)
    return _ro(dict(hd=hd, E=E, W=W, T_l=T_l, B=B, task=task, h=h, Wh=Wh, dout=dout))


@functools.lru_cache(maxsize=None)
def action_grad_case(A, E, Wc, B, seed=0):
    """dz1 whose rows are zero where dq is (so the compacted and the dense form see the same sums), the critic's
    layer-0 kernel with Ic = A + 5 input rows, a policy cache with log-stds at and beyond the bounds, saturated
    actions, eps of 0 and +-4, and logged actions a_data that equal a in row 0."""
    rng = np.random.default_rng(4000 * A + 100 * E + Wc + 7 * B + seed)
    dq = rng.standard_normal((E, B)).astype(f32)
    dq[rng.uniform(size=(E, B)) < 0.4] = 0.0
    dq[:, 1::5] = -0.0
    dz1 = rng.standard_normal((E, B, Wc)).astype(f32)
    dz1[dq == 0] = 0.0
    Ic = A + 5
    W0 = (rng.standard_normal((E, Ic, Wc)) / np.sqrt(Wc)).astype(f32)
    mu = rng.standard_normal((B, A)).astype(f32)
    ls = rng.uniform(LS_MIN - 0.5, LS_MAX + 0.5, (B, A)).astype(f32)
    ls.flat[0::6] = LS_MAX
    ls.flat[1::6] = LS_MIN
    eps = rng.standard_normal((B, A)).astype(f32)
    eps.flat[2::7] = 0.0
    eps.flat[3::11] = 4.0
    eps.flat[4::13] = -4.0
    x = (mu + np.exp(np.clip(ls, LS_MIN, LS_MAX)) * eps).astype(f32)
    a = np.tanh(x).astype(f32)
    a.flat[5::9] = 1.0
    a.flat[6::9] = -1.0
    cache = np.concatenate([mu, ls, x, a, eps], axis=1).astype(f32)
    ld = A + 2
    a_data = rng.uniform(-1, 1, (B, ld)).astype(f32)
    a_data[0, :A] = a[0]
    return _ro(dict(A=A, E=E, Wc=Wc, B=B, Ic=Ic, dq=dq, dz1=dz1, W0=W0, cache=cache, ld=ld, a_data=a_data,
                    alpha_w=rng.uniform(0.0, 0.02, B).astype(f32), row_loss=rng.standard_normal(B).astype(f32),
                    explore_scale=f32(2.0 / (B * A))))
