"""CPU tests of the optimizer tests' own reference (adam_ref.py, grad_mag_ref.py): it equals the
oracle's and torch's Adam, its moment generator stays inside the bound split2h relies on, the
tolerance rule of test_gpu_optimizer.py catches every seeded optimizer error, and the per-leaf
gradient allowance holds for the float32 oracle with room to spare."""

from __future__ import annotations

import numpy as np
import pytest

import adam_ref as ar
import grad_mag_ref as gm
import sac_opt_cases as sc
from oracle import mtsac as om


def _vectors(n=257, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)
    p = rng.uniform(-0.3, 0.3, n)
    hp = ar.Hyper(lr=1e-3, b1=0.8, b2=0.99, eps=3e-4, tau=0.05)
    mu, nu = ar.reachable_moments(g, hp, seed=1)
    return p, g, mu.astype(np.float64), nu.astype(np.float64), hp


@pytest.mark.parametrize("max_norm", [None, 1e-3, 10.0, 0.0])
@pytest.mark.parametrize("k0", [0, 9, 99999])
def test_reference_equals_oracle(max_norm, k0):
    p, g, mu, nu, hp = _vectors()
    ref = ar.step(p, g, mu, nu, k0, hp, max_norm)
    want_g = om.clip_by_global_norm(g, None if max_norm is None else ar.f32(max_norm))
    st = om.AdamState(mu.copy(), nu.copy(), k0)
    want_p = om.adam_step(p, want_g, st, hp.lr, hp.b1, hp.b2, hp.eps)
    for got, want in ((ref.g_c, want_g), (ref.mu, st.mu), (ref.nu, st.nu), (ref.p, want_p)):
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    assert ref.count == st.count and ref.clipped == (max_norm is not None and max_norm < 1.0)
    assert abs(ref.gnorm - om.global_norm(g)) <= 1e-14 * ref.gnorm


def test_five_steps_equal_torch_adam():
    import torch

    p, _, _, _, hp = _vectors()
    rng = np.random.default_rng(5)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps)
    mu, nu = np.zeros_like(p), np.zeros_like(p)
    for k0 in range(5):
        g = rng.standard_normal(p.size) * 1e-2
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, mu, nu, _ = ar.adam(p, g, mu, nu, k0, hp)
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-15)
    st = opt.state[tp]
    np.testing.assert_allclose(mu, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(nu, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_polyak_is_incremental_update():
    a, b = np.array([1.0, -2.0]), np.array([3.0, 5.0])
    t = ar.f32(0.005)
    np.testing.assert_array_equal(ar.polyak(a, b, 0.005), t * a + (1 - t) * b)


@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.8, 0.99)])
@pytest.mark.parametrize("steps", [1, 4, 40])
def test_generated_moments_are_reachable(b1, b2, steps):
    hp = ar.Hyper(b1=b1, b2=b2)
    g = 10.0 ** np.random.default_rng(2).uniform(-8, 0, 4096)
    mu, nu = ar.reachable_moments(g, hp, seed=3, steps=steps)
    assert mu.dtype == np.float32 and nu.dtype == np.float32 and np.all(nu >= 0) and np.any(mu != 0)
    C = ar.moment_ratio_bound(hp.b1, hp.b2)
    # the float32 casts move each side by one rounding
    assert np.all(np.abs(mu.astype(np.float64)) <= C * np.sqrt(nu.astype(np.float64)) * (1 + 4 * ar.U24))
    # and an arbitrary pair is not inside it: the bound is a property of the generator, not of Adam states
    assert 1.0 > C * np.sqrt(1e-12)


def test_moment_ratio_bound_is_the_engines_without_margin():
    """engine.cpp adam_step_bound_of = 1.25 r C with r = max_t sqrt(1 - b2^t) / (1 - b1^t) >= 1; at the
    defaults r = 1 and the comment there gives r C = 7.27."""
    assert abs(ar.moment_ratio_bound(0.9, 0.999) - 7.27) < 0.005


# ---------------------------------------------------------------------------- seeded errors
def _critic_inputs(name, hset, clip):
    o = sc.oracle_pass(name)
    hs = sc.hyper_set(name, hset)
    st = sc.base_state(name)[0]
    mu, nu = sc.start_moments(name, hs)["critic"]
    return (st.critic, o["critic_grad"], mu.astype(np.float64), nu.astype(np.float64), hs.counts[1],
            hs, sc.clip_thresholds(name, clip)[1], st.critic_target)


SEEDED = {
    # name: (hyper set, clip, quantities that must move, the wrong step)
    "eps_1e-8": ("b", "none", ("p",), lambda a, hp, mx, hs: ar.step(*a[:5], ar.Hyper(hp.lr, hp.b1, hp.b2, 1e-8, hp.tau), mx, a[5])),
    "eps_1e-8_set_c": ("c", "none", ("p",), lambda a, hp, mx, hs: ar.step(*a[:5], ar.Hyper(hp.lr, hp.b1, hp.b2, 1e-8, hp.tau), mx, a[5])),
    # no bias correction: 1 - b^k = 1, which a count of 10^9 gives exactly
    "no_bias_correction": ("b", "none", ("p",), lambda a, hp, mx, hs: ar.step(*a[:4], 10 ** 9, hp, mx, a[5])),
    "b2_for_b1": ("b", "none", ("mu", "p"), lambda a, hp, mx, hs: ar.step(*a[:5], ar.Hyper(hp.lr, hp.b2, hp.b2, hp.eps, hp.tau), mx, a[5])),
    "actor_lr_for_critic": ("c", "none", ("p",), lambda a, hp, mx, hs: ar.step(*a[:5], ar.Hyper(hs.actor_lr, hp.b1, hp.b2, hp.eps, hp.tau), mx, a[5])),
    "tau_off_10_percent": ("b", "none", ("target",), lambda a, hp, mx, hs: ar.step(*a[:5], ar.Hyper(hp.lr, hp.b1, hp.b2, hp.eps, 1.1 * hp.tau), mx, a[5])),
    "clip_factor_1": ("b", "quarter", ("mu", "nu", "p"), lambda a, hp, mx, hs: ar.step(*a[:5], hp, None, a[5])),
}


@pytest.mark.parametrize("name", sc.SMALL)
@pytest.mark.parametrize("error", list(SEEDED))
def test_tolerance_rule_catches_seeded_error(error, name):
    """An engine that computed the wrong step exactly would differ from the reference by more than twice
    the allowance 4 c 2^-24 S (so its own rounding, itself inside the allowance, cannot hide it) in each
    quantity the error touches."""
    hset, clip, quantities, wrong = SEEDED[error]
    p, g, mu, nu, k0, hs, mx, tgt = _critic_inputs(name, hset, clip)
    hp = hs.hyper("critic")
    ref, _, S, c = ar.yardstick(p, g, mu, nu, k0, hp, mx, tgt)
    bad = wrong((p, g, mu, nu, k0, tgt), hp, mx, hs)
    for q in quantities:
        tol = 4 * c[q] * ar.U24 * S[q]
        d = np.abs(getattr(bad, q) - getattr(ref, q))
        assert np.any(d > 2 * tol), (error, name, q, float(np.max(d / np.maximum(tol, 1e-300))))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_yardstick_is_a_few_units(name):
    """The scales are right when numpy float32 stays within a few units of them at every case and set:
    far more would mean a term is missing (the 4x allowance then hides real errors), far less than one
    everywhere that a scale is padded."""
    for hset in ("a", "b", "c") if name in sc.SMALL else ("b",):
        for clip in ("none", "quarter"):
            p, g, mu, nu, k0, hs, mx, tgt = _critic_inputs(name, hset, clip)
            _, _, _, c = ar.yardstick(p, g, mu, nu, k0, hs.hyper("critic"), mx, tgt)
            for q, v in c.items():
                assert v <= 4.0, (name, hset, clip, q, v)


# ---------------------------------------------------------------------------- gradient allowance
@pytest.mark.parametrize("name,clip_tw", [(n, False) for n in sc.CASES] + [("tiny", True)])
def test_float32_oracle_meets_the_leaf_allowance(name, clip_tw):
    """The oracle run in float32 (plain numpy matmuls, no compensated sums) differs from float64 by less
    than a quarter of 1e-5 mag at every element of every leaf.  Against the plain product |in|^T |dz| it
    does not (up to 5.9e-5 at these batch sizes; grad_mag_ref's docstring says why)."""
    o = sc.oracle_pass(name, clip_tw=clip_tw)
    cfg = o["cfg"]
    st, batch, en, ec = sc.base_state(name)[:4]
    s32 = om.MTSACState(*(getattr(st, k).astype(np.float32) for k in ("actor", "critic", "critic_target", "log_alpha")),
                        *(om.AdamState.zeros(n, np.float32) for n in (st.actor.size, st.critic.size, st.log_alpha.size)))
    _, _, lo = om.update(cfg, s32, list(batch), en, ec, return_internals=True)
    for net, shapes in (("critic", om.critic_leaf_shapes(cfg)), ("actor", om.actor_leaf_shapes(cfg))):
        for leaf, worst, exact in gm.leaf_report(lo[net + "_grad"], o[net + "_grad"], o["mag_" + net], shapes):
            assert exact and worst <= 0.25 * gm.GRAD_RTOL, (name, net, leaf, worst)
