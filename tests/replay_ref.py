"""Plain numpy statements of what the replay kernels compute (mtrl_amd/csrc/replay.hip): the gather from the
record store and the scatter of a user batch into the padded GEMM inputs and their planes, the per-task row
lists, the slot pack / commit, the absolute maximum and the synthetic fill.  Everything here is exact (the kernels
move floats, compare them and take maxima); the two places with arithmetic are the normalised reward, one
float64 expression rounded once to float32, and the synthetic fill's normals (tests/philox_ref.py, with its bound).

An element the kernels must leave alone is the all-ones word in the float outputs (a NaN: `untouched`), -1 in the
int outputs and UNTOUCHED (0xFFFF) in the 16-bit plane words: what the guarded debug outputs start as.  The plane
formats are trunk_bias_ref's.
"""

from __future__ import annotations

import numpy as np

import philox_ref as P
from trunk_bias_ref import UNTOUCHED, bf16_words, plane_exp, split2h, split3

f32 = np.float32


def untouched(*shape):
    """float32 all-ones words (a NaN): what a guarded output holds where no kernel wrote."""
    return np.full(shape, 0xFFFFFFFF, np.uint32).view(f32)


def record_width(D, A):
    return (2 * D + A + 2 + 3) // 4 * 4


def pack_records(obs, act, rew, done, nobs, R=None, pad=0.0):
    """[..., R] records [obs | act | rew | done | next_obs | pad] from arrays with matching leading dimensions."""
    D, A = obs.shape[-1], act.shape[-1]
    R = record_width(D, A) if R is None else R
    rec = np.full(obs.shape[:-1] + (R,), pad, f32)
    rec[..., :D] = obs
    rec[..., D:D + A] = act
    rec[..., D + A] = rew
    rec[..., D + A + 1] = done
    rec[..., D + A + 2:2 * D + A + 2] = nobs
    return rec


def unpack_rows(store, idx, D, A):
    """The five batch arrays (rows i T_l + t) of the sampled slots."""
    rows = store[np.asarray(idx)].reshape(-1, store.shape[-1])
    return (rows[:, :D], rows[:, D:D + A], rows[:, D + A + 2:2 * D + A + 2], rows[:, D + A + 1], rows[:, D + A])


def one_hot_task(obs, nobs, T_glob, task_begin, T_l):
    """(task [B], err): the gather's one-hot check on the last T_glob columns of obs and next_obs.  A row passes
    when each holds exactly one 1.0 and otherwise only (+-)0.0, both at the same column, of a local task."""
    B, D = obs.shape
    task, err = np.zeros(B, np.int32), 0
    for b in range(B):
        o, n = obs[b, D - T_glob:], nobs[b, D - T_glob:]
        ok = True
        for v in (o, n):
            ones = v == 1.0
            ok &= int(ones.sum()) == 1 and not np.any(~ones & ~(v == 0.0))  # NaN is neither: a bad entry
        if ok:
            fo, fn = int(np.argmax(o == 1.0)), int(np.argmax(n == 1.0))
            local = fo - task_begin
            ok = fo == fn and 0 <= local < T_l
        if ok:
            task[b] = local
        else:
            err = 1
    return task, err


def normalised_reward(rew, t, rmin, rmax, eps):
    r = rew.astype(np.float64)
    return ((r - rmin[t]) / (rmax[t] - rmin[t] + eps)).astype(f32)


def _put(words, rows, col0, x, mode, e):
    """x [len(rows)][w] into the plane words [np][rows allocated][ld] at (rows, col0 ..)."""
    with np.errstate(over="ignore"):  # a value past the bound the exponent was taken from is fp16 inf, as on the device
        parts = [bf16_words(p) for p in split3(x)] if mode == 1 else list(split2h(x, e))
    for q, w in enumerate(parts):
        words[q][np.asarray(rows)[:, None], col0 + np.arange(x.shape[1])[None, :]] = w


def gather_model(obs, act, nobs, done, rew, T_l, T_glob, task_begin, ld_a, ld_c, plane_mode=0, pa_ld=0, pc_ld=0,
                 pa_next=0, pa_rows=0, pc_rows=0, in_max=None, rmin=None, rmax=None, norm_eps=0.0):
    """Every output of gather_kernel for the batch rows given (row b of local task b % T_l)."""
    obs, act, nobs = (np.ascontiguousarray(x, f32) for x in (obs, act, nobs))
    B, D = obs.shape
    A = act.shape[1]
    o = {k: untouched(B, ld_a) for k in ("xa", "xa_next")}
    o.update({k: untouched(B, ld_c) for k in ("xc", "xc_next", "xc_pi")})
    o["xa"][:, :D], o["xa_next"][:, :D] = obs, nobs
    o["xc"][:, :A], o["xc"][:, A:A + D] = act, obs
    o["xc_pi"][:, A:A + D], o["xc_next"][:, A:A + D] = obs, nobs
    t = np.arange(B) % T_l
    o["rew"] = np.asarray(rew, f32).copy() if rmin is None else normalised_reward(np.asarray(rew, f32), t, rmin, rmax, norm_eps)
    o["done"] = np.asarray(done, f32).copy()
    o["task"], o["err"] = one_hot_task(obs, nobs, T_glob, task_begin, T_l)
    if plane_mode:
        np_ = 2 if plane_mode == 2 else 3
        e = plane_exp(max(float(f32(in_max)), 1.0)) if plane_mode == 2 else 0
        if plane_mode == 2:
            o["e"] = e  # in_rec->e
        o["pa"] = np.full((np_, pa_rows, pa_ld), UNTOUCHED, np.uint16)
        for k in ("pc", "pcn", "pcp"):
            o[k] = np.full((np_, pc_rows, pc_ld), UNTOUCHED, np.uint16)
        rows = np.arange(B)
        _put(o["pa"], rows, 0, obs, plane_mode, e)
        _put(o["pa"], pa_next + rows, 0, nobs, plane_mode, e)
        _put(o["pc"], rows, 0, act, plane_mode, e)
        _put(o["pc"], rows, A, obs, plane_mode, e)
        _put(o["pcp"], rows, A, obs, plane_mode, e)
        _put(o["pcn"], rows, A, nobs, plane_mode, e)
    return o


# ------------------------------------------------------------------ row lists, pack / commit, absmax
def task_rows_model(task, T_l, max_rows):
    task = np.asarray(task)
    counts = np.bincount(task, minlength=T_l).astype(np.int32)
    rows = np.full((T_l, max_rows), -1, np.int32)
    for t in range(T_l):
        r = np.flatnonzero(task == t)[:max_rows]  # ascending; the overflow is dropped
        rows[t, :len(r)] = r
    return counts, rows


def stored_absmax(rec, D, A):
    """max |obs|, |action|, |next_obs| of records [..., R]: the reward and done columns and the pad do not count."""
    return float(max(np.abs(rec[..., :D + A]).max(), np.abs(rec[..., D + A + 2:2 * D + A + 2]).max()))


def pack_commit_model(obs, nobs, act, rew, done, R, rmin, rmax, bufmax):
    D, A = obs.shape[1], act.shape[1]
    rec = pack_records(obs, act, rew, done, nobs, R)
    r64 = np.asarray(rew, f32).astype(np.float64)
    return rec, np.minimum(rmin, r64), np.maximum(rmax, r64), f32(max(float(bufmax), stored_absmax(rec, D, A)))


def absmax_model(x, m):
    return f32(max(float(m), float(np.abs(x).max())))


# ------------------------------------------------------------------ synthetic fill
def fill_model(cap, T_l, D, A, T_glob, task_begin, seed):
    """(store float64 [cap][T_l][R], bound [cap][T_l][R], exact [R] bool): fill_kernel's records.  Columns with
    exact set are bit for bit (one-hots, uniform actions / reward / done, pad); the others are Box-Muller normals
    held to philox_ref.normal_bound."""
    R, F = record_width(D, A), D - T_glob
    store, bound = np.zeros((cap * T_l, R)), np.zeros((cap * T_l, R))
    exact = np.ones(R, bool)
    exact[:F] = exact[D + A + 2:D + A + 2 + F] = False
    for r in range(cap * T_l):
        t = r % T_l
        for stream, base in ((1, 0), (2, D + A + 2)):
            for c in range(0, F, 4):
                v, rad = P.normal4_model(seed, stream, r, c)
                n = min(4, F - c)
                store[r, base + c:base + c + n], bound[r, base + c:base + c + n] = v[:n], P.normal_bound(rad[:n])
        store[r, F + task_begin + t] = store[r, D + A + 2 + F + task_begin + t] = 1.0
        for c in range(0, A, 4):
            u = P.uniform4(seed, 3, r, c)
            n = min(4, A - c)
            store[r, D + c:D + c + n] = (f32(2.0) * u[:n] - f32(1.0)).astype(f32)
        u = P.uniform4(seed, 4, r, 0)
        store[r, D + A] = f32(10.0) * u[0]
        store[r, D + A + 1] = 1.0 if u[1] < f32(1.0) / f32(500.0) else 0.0
    return store.reshape(cap, T_l, R), bound.reshape(cap, T_l, R), exact
