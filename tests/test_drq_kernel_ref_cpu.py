"""Pins the plain references of tests/drq_kernel_ref.py (what the GPU kernel tests compare against)
on the CPU: the convs and the pool against torch in float64, the C51 trio against the oracle, and
the float32 facts of the projection's discontinuity that the references and the oracle rely on."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import drq_kernel_ref as R
from oracle import drq as od

PAIRS = [(4, 8), (8, 8), (8, 16), (16, 16)]


def _nchw(a):
    return torch.as_tensor(np.asarray(a, np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 2, 2), (2, 3, 7), (2, 11, 6)])
def test_conv_reference_matches_torch(shape):
    B, H, W = shape
    for ci, co in PAIRS:
        rng = np.random.default_rng(ci * 100 + co + H * 7 + W)
        x = rng.standard_normal((B, H, W, ci))
        w = rng.standard_normal((3, 3, ci, co))
        bias, res = rng.standard_normal(co), rng.standard_normal((B, H, W, co))
        dout = rng.standard_normal((B, H, W, co))
        wt = torch.as_tensor(w).permute(3, 2, 0, 1).clone().requires_grad_(True)  # [co][ci][3][3]
        for relu in (False, True):
            xt = _nchw(x).clone().requires_grad_(True)
            y = F.conv2d(torch.relu(xt) if relu else xt, wt, torch.as_tensor(bias), padding=1) + _nchw(res)
            out, S = R.conv_fwd(x, w, bias, relu, res)
            np.testing.assert_allclose(out, _nhwc(y), rtol=1e-12, atol=1e-12)
            assert (S >= np.abs(out) - 1e-12).all()
            gx, gw = torch.autograd.grad(y, (xt, wt), _nchw(dout))
            # the data gradient of conv(relu(x)) is conv^T(dout) [x > 0]
            din, Sd = R.conv_bwd_data(dout, w, x if relu else None)
            np.testing.assert_allclose(din, _nhwc(gx), rtol=1e-12, atol=1e-12)
            assert (Sd >= np.abs(din) - 1e-12).all()
            dw, db, Sw, Sb = R.conv_wgrad(x, dout, relu)
            np.testing.assert_allclose(dw, gw.permute(2, 3, 1, 0).numpy(), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(db, dout.sum((0, 1, 2)), rtol=1e-12, atol=1e-12)
            assert (Sw >= np.abs(dw) - 1e-12).all() and (Sb >= np.abs(db) - 1e-12).all()
        # residual gradient added after the mask; exact zeros of either sign block the gradient
        mask = rng.standard_normal(x.shape)
        mask.flat[::5], mask.flat[1::7] = 0.0, -0.0
        dres = rng.standard_normal(x.shape)
        plain, _ = R.conv_bwd_data(dout, w)
        got, _ = R.conv_bwd_data(dout, w, mask, dres)
        np.testing.assert_array_equal(got, np.where(mask > 0, plain, 0.0) + dres)
        # two parameter sets = the two halves run apart
        w2, b2 = rng.standard_normal(w.shape), rng.standard_normal(co)
        for B1 in range(B + 1):
            both, S2 = R.conv_fwd(x, w, bias, True, res, w2, b2, B1)
            first, _ = R.conv_fwd(x, w, bias, True, res)
            second, _ = R.conv_fwd(x, w2, b2, True, res)
            np.testing.assert_array_equal(both[:B1], first[:B1])
            np.testing.assert_array_equal(both[B1:], second[B1:])


@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (2, 2), (3, 3), (4, 5), (5, 4), (7, 7), (10, 10), (20, 11)])
def test_pool_reference_matches_torch(hw):
    H, W = hw
    B, C = 2, 8
    rng = np.random.default_rng(H * 31 + W)
    x = rng.permutation(B * H * W * C).reshape(B, H, W, C).astype(np.float64)  # tie-free
    (Ho, loy), (Wo, lox) = R.pool_geometry(H), R.pool_geometry(W)
    dout = rng.integers(-3, 4, (B, Ho, Wo, C)).astype(np.float64)
    hiy, hix = (Ho - 1) * 2 + 3 - H - loy, (Wo - 1) * 2 + 3 - W - lox
    xt = _nchw(x).clone().requires_grad_(True)
    y = F.max_pool2d(F.pad(xt, (lox, max(hix, 0), loy, max(hiy, 0)), value=-np.inf), 3, 2)
    assert y.shape[2:] == (Ho, Wo)
    (gx,) = torch.autograd.grad(y, xt, _nchw(dout))
    out, arg, din = R.maxpool(x, dout)
    np.testing.assert_array_equal(out, _nhwc(y))
    np.testing.assert_array_equal(din, _nhwc(gx))
    # arg names the pixel that holds the maximum
    for b, oy, ox, c in np.ndindex(B, Ho, Wo, C):
        t = int(arg[b, oy, ox, c])
        assert x[b, 2 * oy - loy + t // 3, 2 * ox - lox + t % 3, c] == out[b, oy, ox, c]


def test_pool_reference_takes_the_first_maximum():
    x = np.ones((1, 5, 4, 4))
    out, arg, din = R.maxpool(x, np.ones((1, 3, 2, 4)))
    # 5 rows pad 1 in front, 4 columns pad 0: the first in-image tap of each window, row major
    assert arg[0, :, :, 0].tolist() == [[3, 3], [0, 0], [0, 0]]
    assert din.sum() == 3 * 2 * 4 and (out == 1).all()


def _heads(rng, B, A, Z, ldh):
    hc = [(3 * rng.standard_normal((B, ldh))).astype(np.float32) for _ in range(3)]
    hb = [rng.standard_normal((A + 1) * Z).astype(np.float32) for _ in range(2)]
    return hc, hb


def test_c51_reference_matches_oracle_at_51_atoms():
    B, A, Z = 6, 18, 51
    cfg = od.DrQConfig(n_actions=A, n_atoms=Z)
    rng = np.random.default_rng(3)
    (hs, hn, ht), (bo, bt) = _heads(rng, B, A, Z, (A + 1) * Z)
    rew = np.array([0.3, -1.7, 25.0, -25.0, 0.0, 4.0], np.float32)
    done = np.array([0, 0, 0, 0, 1, 1], np.float32)
    act = rng.integers(0, A, B)
    m, a_next, q, dh, loss_b, logit_b = R.c51(hs, hn, ht, bo, bt, rew, done, act, A, Z, cfg.gamma, cfg.nstep,
                                              cfg.v_min, cfg.v_max)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    lo, lt = t(R.head_logits(hn, bo, A, Z)), t(R.head_logits(ht, bt, A, Z))
    m_o, a_o = od.c51_target(lo, lt, t(rew), t(done), cfg)
    np.testing.assert_array_equal(a_next, a_o.numpy())
    np.testing.assert_allclose(m, m_o.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.sum(-1)[0], 1.0, atol=1e-12)  # no atom of row 0 is clamped: nothing dropped
    # loss and gradient against autograd on the same m
    hs_t = t(hs).clone().requires_grad_(True)
    h = hs_t + t(bo)
    adv, val = h[:, :A * Z].reshape(B, A, Z), h[:, A * Z:].reshape(B, 1, Z)
    logits = (val + (adv - adv.mean(1, keepdim=True)))[torch.arange(B), torch.as_tensor(act)]
    lb = -(t(m) * torch.log_softmax(logits, -1)).sum(-1)
    (g,) = torch.autograd.grad(lb.mean(), hs_t)
    np.testing.assert_allclose(loss_b, lb.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dh, g.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(logit_b, logits.sum(-1).detach().numpy(), rtol=1e-12)
    sup = np.linspace(cfg.v_min, cfg.v_max, Z)
    np.testing.assert_allclose(q, (torch.softmax(lo, -1).numpy() * sup).sum(-1), rtol=0, atol=1e-5)


@pytest.mark.parametrize("Z", [2, 33, 40, 59, 62, 64])
def test_oracle_projection_is_the_float32_one(Z):
    """oracle.drq.c51_target decides floor / ceil as the reference does, at every atom count."""
    B, A = 6, 3
    cfg = od.DrQConfig(n_actions=A, n_atoms=Z)
    rng = np.random.default_rng(Z)
    (hs, hn, ht), (bo, bt) = _heads(rng, B, A, Z, (A + 1) * Z)
    rew = np.array([0.3, -1.7, 25.0, -25.0, 0.0, 10.0], np.float32)
    done = np.array([0, 0, 0, 0, 1, 1], np.float32)
    m, a_next, *_ = R.c51(hs, hn, ht, bo, bt, rew, done, np.zeros(B, int), A, Z, cfg.gamma, cfg.nstep, cfg.v_min,
                          cfg.v_max)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    m_o, a_o = od.c51_target(t(R.head_logits(hn, bo, A, Z)), t(R.head_logits(ht, bt, A, Z)), t(rew), t(done), cfg)
    np.testing.assert_array_equal(a_next, a_o.numpy())
    np.testing.assert_allclose(m, m_o.numpy(), rtol=0, atol=1e-12)


def test_projection_float32_facts():
    """A clamped top atom (tz = v_max) has b = (v_max - v_min) / dz: in float32 just below Z - 1 at 64
    and 40 atoms (the mass is kept, on the last atom), exactly integral in float64 there (dropped);
    float64 is itself off at 30, 54, 59 and 62 atoms, and at 62 its ceil is past the last atom."""
    vmin, vmax, g, n = -10.0, 10.0, 0.99, 3
    for Z, want in ((64, "62.999996"), (40, "38.999996")):
        _, b, l, u = R.c51_index_f32([25.0], [0.0], Z, g, n, vmin, vmax)
        assert str(b[0, -1]) == want and (l[0, -1], u[0, -1]) == (Z - 2, Z - 1), (Z, b[0, -1])
        assert (vmax - vmin) / ((vmax - vmin) / (Z - 1)) == Z - 1  # float64: integral, l == u
        # so the reference keeps the whole distribution of a row clamped high
        (hs, hn, ht), (bo, bt) = _heads(np.random.default_rng(Z), 1, 2, Z, 3 * Z)
        m, *_ = R.c51(hs, hn, ht, bo, bt, [25.0], [0.0], [0], 2, Z, g, n, vmin, vmax)
        assert abs(m.sum() - 1.0) < 1e-6 and m[0, Z - 1] > 0.99
    for Z in (30, 54, 59, 62):
        b64 = (vmax - vmin) / ((vmax - vmin) / (Z - 1))
        assert b64 != Z - 1, Z
        _, b, l, u = R.c51_index_f32([25.0], [0.0], Z, g, n, vmin, vmax)
        assert b[0, -1] == Z - 1 and l[0, -1] == u[0, -1] == Z - 1, Z  # float32: integral, dropped
    assert np.ceil((vmax - vmin) / ((vmax - vmin) / 61)) == 62  # past the last of 62 atoms
    # reward 0, done 1 at 59 atoms: tz = 0, b = 10 / dz
    _, b, l, u = R.c51_index_f32([0.0], [1.0], 59, g, n, vmin, vmax)
    b64 = (0.0 - vmin) / ((vmax - vmin) / 58)
    assert (l[0, 0] == u[0, 0]) != (np.floor(b64) == np.ceil(b64))
    # at 51 atoms the two precisions agree on every clamped row
    _, b, l, u = R.c51_index_f32([25.0, -25.0], [0.0, 0.0], 51, g, n, vmin, vmax)
    assert (l == u).all() and (l[0] == 50).all() and (l[1] == 0).all()
    assert (vmax - vmin) / ((vmax - vmin) / 50) == 50.0


def test_kernel_dz_is_the_reference_dz():
    """c51_target_kernel forms dz = (vmax - vmin) / (float)(Z - 1) in float32 from the float32 bounds
    of drq_config; the reference rounds the double quotient once.  They must be the same number for
    every atom count drq_create takes (bounds that float32 holds exactly, as the config stores them)."""
    f = np.float32
    for vmin, vmax in ((-10.0, 10.0), (0.0, 200.0), (-1.0, 1.0), (-7.5, 12.25), (-0.5, 0.5), (-100.0, 300.0)):
        for Z in range(2, 65):
            kernel = (f(vmax) - f(vmin)) / f(Z - 1)
            ref = f((vmax - vmin) / (Z - 1))
            assert kernel == ref, (vmin, vmax, Z, kernel, ref)
