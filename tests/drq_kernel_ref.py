"""Plain float64 references of single DrQ kernels (mtrl_amd/csrc/drq.hip), written as the
definitions: loops / einsum over the taps, no tricks.  tests/test_drq_kernel_ref_cpu.py pins them
against torch; tests/test_gpu_drq_kernels.py holds the kernels to them.

Layouts are the engine's: images NHWC, conv kernels [3][3][ci][co], 3 x 3 / stride 1 / SAME.
Each conv reference also returns S = the sum of the |terms| of every output (the analogue of `mag`
in tests/test_gpu_kernels.py), the scale an fp32 evaluation's rounding is measured against."""

import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _pad1(a):
    return np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))


# ---------------------------------------------------------------- convolutions
def conv_fwd(x, w, bias, relu_in=False, res=None, w2=None, bias2=None, B1=None):
    """out[b,y,x,o] = bias[o] + sum_{dy,dx,c} act(x)[b,y+dy-1,x+dx-1,c] w[dy,dx,c,o] (+ res);
    images [B1, B) take (w2, bias2).  Returns (out, S)."""
    x, w, bias, res, w2, bias2 = (_f64(a) for a in (x, w, bias, res, w2, bias2))
    B, H, W, _ = x.shape
    a = np.maximum(x, 0.0) if relu_in else x
    ap = _pad1(a)
    out = np.zeros((B, H, W, w.shape[-1]))
    S = np.zeros_like(out)
    for b in range(B):
        wb, bb = (w2, bias2) if (w2 is not None and B1 is not None and b >= B1) else (w, bias)
        out[b] += bb
        S[b] += np.abs(bb)
        for dy in range(3):
            for dx in range(3):
                win = ap[b, dy:dy + H, dx:dx + W, :]
                out[b] += np.einsum("yxc,co->yxo", win, wb[dy, dx])
                S[b] += np.einsum("yxc,co->yxo", np.abs(win), np.abs(wb[dy, dx]))
    if res is not None:
        out += res
        S += np.abs(res)
    return out, S


def conv_bwd_data(dout, w, mask=None, dres=None):
    """din[b,y,x,c] = (sum_{dy,dx,o} dout[b,y-dy+1,x-dx+1,o] w[dy,dx,c,o]) [mask > 0] (+ dres).
    Returns (din, S)."""
    dout, w, mask, dres = (_f64(a) for a in (dout, w, mask, dres))
    B, H, W, _ = dout.shape
    gp = _pad1(dout)
    din = np.zeros((B, H, W, w.shape[-2]))
    S = np.zeros_like(din)
    for dy in range(3):
        for dx in range(3):
            win = gp[:, 2 - dy:2 - dy + H, 2 - dx:2 - dx + W, :]  # dout[y - dy + 1][x - dx + 1]
            din += np.einsum("byxo,co->byxc", win, w[dy, dx])
            S += np.einsum("byxo,co->byxc", np.abs(win), np.abs(w[dy, dx]))
    if mask is not None:
        keep = mask > 0  # strictly: 0.0 and -0.0 block the gradient
        din = np.where(keep, din, 0.0)
        S = np.where(keep, S, 0.0)
    if dres is not None:
        din = din + dres
        S = S + np.abs(dres)
    return din, S


def conv_wgrad(x, dout, relu_in=False):
    """dw[dy,dx,c,o] = sum_{b,y,x} act(x)[b,y+dy-1,x+dx-1,c] dout[b,y,x,o], db[o] = sum dout.
    Returns (dw, db, S_dw, S_db)."""
    x, dout = _f64(x), _f64(dout)
    B, H, W, ci = x.shape
    a = np.maximum(x, 0.0) if relu_in else x
    ap = _pad1(a)
    dw = np.zeros((3, 3, ci, dout.shape[-1]))
    S = np.zeros_like(dw)
    for dy in range(3):
        for dx in range(3):
            win = ap[:, dy:dy + H, dx:dx + W, :]
            dw[dy, dx] = np.einsum("byxc,byxo->co", win, dout)
            S[dy, dx] = np.einsum("byxc,byxo->co", np.abs(win), np.abs(dout))
    return dw, dout.sum((0, 1, 2)), S, np.abs(dout).sum((0, 1, 2))


# ---------------------------------------------------------------- max pool 3 x 3 / stride 2 / SAME
def pool_geometry(n):
    """(outputs, padding before the first element) of one axis: SAME splits the total padding
    max((no - 1) 2 + 3 - n, 0) with the smaller half in front."""
    no = (n + 1) // 2
    return no, max((no - 1) * 2 + 3 - n, 0) // 2


def maxpool(x, dout):
    """x [B][H][W][C], dout [B][Ho][Wo][C] -> (out, arg, din): arg = the window tap (0..8, row
    major) of the first maximum, din = dout scattered to the argmax pixel."""
    x = _f64(x)
    dout = _f64(dout)
    B, H, W, C = x.shape
    (Ho, loy), (Wo, lox) = pool_geometry(H), pool_geometry(W)
    out = np.full((B, Ho, Wo, C), -np.inf)
    arg = np.zeros((B, Ho, Wo, C), np.uint8)
    din = np.zeros_like(x)
    ch = np.arange(C)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for tap in range(9):
                    y, xx = 2 * oy - loy + tap // 3, 2 * ox - lox + tap % 3
                    if not (0 <= y < H and 0 <= xx < W):
                        continue
                    better = x[b, y, xx] > out[b, oy, ox]  # strictly: the first maximum stays
                    out[b, oy, ox][better] = x[b, y, xx][better]
                    arg[b, oy, ox][better] = tap
                t = arg[b, oy, ox].astype(int)
                np.add.at(din[b], (2 * oy - loy + t // 3, 2 * ox - lox + t % 3, ch), dout[b, oy, ox])
    return out, arg, din


# ---------------------------------------------------------------- dueling head + C51
def head_logits(hc, hb, A, Z):
    """[B][ldh] head output (+ bias [(A + 1) Z]) -> logits [B][A][Z] = val + adv - mean_a adv."""
    h = _f64(hc)[:, :(A + 1) * Z] + _f64(hb)
    adv, val = h[:, :A * Z].reshape(-1, A, Z), h[:, A * Z:].reshape(-1, 1, Z)
    return val + (adv - adv.mean(1, keepdims=True))


def _softmax(l):
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def c51_index_f32(rew, done, Z, gamma, nstep, vmin, vmax):
    """The discontinuous part of the projection in the reference's precision (drqeps.py
    _update_inner runs it on float32 arrays): support, tz, b, floor, ceil in float32, in its order.
    delta_z and gamma ** nstep are Python doubles there and meet the float32 arrays as weakly
    typed scalars, i.e. rounded once to float32.  Returns (support, b, l, u), l / u int64."""
    f = np.float32
    dz = f((vmax - vmin) / (Z - 1))
    sup = (f(vmin) + np.arange(Z, dtype=f) * dz).astype(f)  # linspace: start + i step
    gn = f(gamma ** nstep)
    rew, done = np.asarray(rew, f).reshape(-1, 1), np.asarray(done, f).reshape(-1, 1)
    tz = np.clip(rew + (gn * (f(1) - done)) * sup, f(vmin), f(vmax)).astype(f)
    b = ((tz - f(vmin)) / dz).astype(f)
    return sup, b, np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)


def c51(hc_s, hc_n, hc_t, hb_on, hb_tg, rew, done, act, A, Z, gamma, nstep, vmin, vmax):
    """The kernels' trio: target m [B][Z] and a_next from (hc_n online, hc_t target); q [B][A] of
    hc_n; loss at `act` from hc_s and m: dh [B][ldh] (zeros past (A + 1) Z), loss_b, logit_b.
    Everything but c51_index_f32 is float64.  l == u drops its mass (both weights are 0) and a
    scatter target past the last atom is dropped, as jax's .at[].add does."""
    B, ldh = np.shape(hc_s)
    sup32, b32, l, u = c51_index_f32(rew, done, Z, gamma, nstep, vmin, vmax)
    sup, b = sup32.astype(np.float64), b32.astype(np.float64)
    q = (_softmax(head_logits(hc_n, hb_on, A, Z)) * sup).sum(-1)
    a_next = q.argmax(-1)  # first maximum
    p = _softmax(head_logits(hc_t, hb_tg, A, Z))[np.arange(B), a_next]
    m = np.zeros((B, Z))
    for i in range(B):
        for j in range(Z):
            if l[i, j] < Z:
                m[i, l[i, j]] += p[i, j] * (u[i, j] - b[i, j])
            if u[i, j] < Z:
                m[i, u[i, j]] += p[i, j] * (b[i, j] - l[i, j])
    act = np.asarray(act, np.int64)
    ls = head_logits(hc_s, hb_on, A, Z)[np.arange(B), act]
    mx = ls.max(-1, keepdims=True)
    logp = ls - (mx + np.log(np.exp(ls - mx).sum(-1, keepdims=True)))
    loss_b = -(m * logp).sum(-1)
    logit_b = ls.sum(-1)
    g = (np.exp(logp) * m.sum(-1, keepdims=True) - m) / B  # d mean_b(loss) / d logit[act]
    dh = np.zeros((B, ldh))
    for a in range(A):
        dh[:, a * Z:(a + 1) * Z] = g * ((act == a).astype(np.float64)[:, None] - 1.0 / A)
    dh[:, A * Z:(A + 1) * Z] = g
    return m, a_next, q, dh, loss_b, logit_b
