"""Float64 reference of the SAC optimizer step (mtrl_amd/csrc/optim.hip) on flat vectors, and the
pieces the optimizer tests share: a float32 evaluation of the same formulas (the yardstick), per-element
error scales, and a generator of reachable Adam moments.

The step is optax.chain(clip_by_global_norm(max), adam(lr, b1, b2, eps)) + apply_updates, then
optax.incremental_update for a Polyak target:

    g_c  = g                      if max is None or ||g|| < max, else (g / ||g||) max
    mu'  = (1 - b1) g_c + b1 mu         nu' = (1 - b2) g_c^2 + b2 nu        k = k0 + 1
    u    = (mu' / (1 - b1^k)) / (sqrt(nu' / (1 - b2^k)) + eps)
    p'   = p - lr u                     target' = tau p' + (1 - tau) target

Every hyper-parameter is rounded to float32 first: the engine receives them as C floats, so the value
it computes with is float32(0.9), not 0.9.

Error scales.  A float32 implementation of these formulas cannot be compared with float64 at a fixed
relative tolerance: mu' = (1 - b1) g + b1 mu cancels, 1 - b2^k loses digits while b2^k is near 1, and
p' carries p's rounding beside the step's.  `scales` gives, per element and quantity, the sum of the
absolute terms of the formula with every upstream term's own scale carried along, so that a faithful
float32 evaluation in any operation order errs by a small multiple of 2^-24 times the scale.  The tests
measure that multiple for numpy float32 (`yardstick`) and allow the engine 4 times it.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

U24 = 2.0 ** -24  # float32 unit roundoff


def f32(x) -> float:
    """The float64 value of x rounded to float32."""
    return float(np.float32(x))


@dataclasses.dataclass
class Hyper:
    lr: float = 3e-4
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-5
    tau: float = 0.005

    def __post_init__(self):
        for f in dataclasses.fields(self):
            setattr(self, f.name, f32(getattr(self, f.name)))


@dataclasses.dataclass
class Step:
    g_c: np.ndarray
    mu: np.ndarray
    nu: np.ndarray
    u: np.ndarray
    p: np.ndarray
    target: np.ndarray | None
    gnorm: float
    clipped: bool
    count: int


def global_norm(g, dtype=np.float64):
    g = np.asarray(g, dtype)
    return np.sqrt(np.sum(g * g))


def clip_by_global_norm(g, max_norm, dtype=np.float64):
    """optax.clip_by_global_norm: g if ||g|| < max, else (g / ||g||) * max; None: no clip in the chain."""
    g = np.asarray(g, dtype)
    if max_norm is None:
        return g
    n = global_norm(g, dtype)
    if n < dtype(f32(max_norm)):
        return g
    return (g / n) * dtype(f32(max_norm))


def adam(p, g, mu, nu, k0: int, hp: Hyper, dtype=np.float64):
    """One optax.adam step + apply_updates with counts k0 -> k0 + 1; returns (p', mu', nu', u)."""
    p, g, mu, nu = (np.asarray(x, dtype) for x in (p, g, mu, nu))
    one, b1, b2 = dtype(1), dtype(hp.b1), dtype(hp.b2)
    k = k0 + 1
    mu = (one - b1) * g + b1 * mu
    nu = (one - b2) * (g * g) + b2 * nu
    bc1 = one - np.power(b1, dtype(k))
    bc2 = one - np.power(b2, dtype(k))
    u = (mu / bc1) / (np.sqrt(nu / bc2) + dtype(hp.eps))
    return p + u * dtype(-hp.lr), mu, nu, u


def polyak(p_new, target, tau, dtype=np.float64):
    """optax.incremental_update(new, old, tau) = tau new + (1 - tau) old."""
    t = dtype(f32(tau))
    return t * np.asarray(p_new, dtype) + (dtype(1) - t) * np.asarray(target, dtype)


def step(p, g, mu, nu, k0: int, hp: Hyper, max_norm, target=None, dtype=np.float64) -> Step:
    """clip + Adam (+ Polyak) of one network."""
    g = np.asarray(g, dtype)
    gn = global_norm(g, dtype)
    g_c = clip_by_global_norm(g, max_norm, dtype)
    p1, mu1, nu1, u = adam(p, g_c, mu, nu, k0, hp, dtype)
    t1 = None if target is None else polyak(p1, target, hp.tau, dtype)
    return Step(g_c, mu1, nu1, u, p1, t1, float(gn), g_c is not g, k0 + 1)


def scales(p, mu, nu, k0: int, hp: Hyper, ref: Step, target=None) -> dict:
    """Per-element error scales (float64) of mu', nu', p' and target' for the float64 result `ref`.

    mu': (1 - b1) w |g_c| + b1 |mu|, with w = 1 unclipped (g itself is known to one rounding: the tests
         recover it from a float32 mu') and 4 clipped (the norm's rounding, the division, the product).
    nu': (1 - b2) 2 w g_c^2 + b2 nu.
    u:   S_mu' / bc1 / (sqrt(nu_hat) + eps) (1 + R1) + |u| (S_nu' / (2 nu') + R2 / 2 + 3), where
         R = (1 + b^k) / (1 - b^k) is the relative error 1 - b^k takes from one rounding of b^k and one of
         the difference, and 3 counts the two divisions, the square root and the sum.
    p':  |p| + lr S_u + lr |u|;   target': tau S_p' + (1 - tau) |target|."""
    p, mu, nu = (np.asarray(x, np.float64) for x in (p, mu, nu))
    k = k0 + 1
    w = 4.0 if ref.clipped else 1.0
    g = np.abs(ref.g_c)
    s_mu = (1 - hp.b1) * w * g + hp.b1 * np.abs(mu)
    s_nu = (1 - hp.b2) * 2 * w * g * g + hp.b2 * nu
    bc1, bc2 = 1 - hp.b1 ** k, 1 - hp.b2 ** k
    r1, r2 = (1 + hp.b1 ** k) / bc1, (1 + hp.b2 ** k) / bc2
    den = np.sqrt(ref.nu / bc2) + hp.eps
    rel_nu = np.divide(s_nu, 2 * ref.nu, out=np.zeros_like(s_nu), where=ref.nu > 0)
    s_u = s_mu / bc1 / den * (1 + r1) + np.abs(ref.u) * (rel_nu + r2 / 2 + 3)
    s_p = np.abs(p) + hp.lr * s_u + hp.lr * np.abs(ref.u)
    out = {"mu": s_mu, "nu": s_nu, "p": s_p}
    if target is not None:
        out["target"] = hp.tau * s_p + (1 - hp.tau) * np.abs(np.asarray(target, np.float64))
    return out


FLOOR = 0.5  # a float32 result is at best correctly rounded: half a unit of its own scale


def yardstick(p, g, mu, nu, k0: int, hp: Hyper, max_norm, target=None):
    """(ref, lo, S, c): the float64 step, the numpy float32 step on the same inputs, the scales, and per
    quantity the largest error of the float32 step in units of 2^-24 S, not below FLOOR (one scalar such
    as 1 - b2^k or the norm can round luckily in numpy and not in another faithful implementation)."""
    ref = step(p, g, mu, nu, k0, hp, max_norm, target)
    lo = step(p, g, mu, nu, k0, hp, max_norm, target, dtype=np.float32)
    S = scales(p, mu, nu, k0, hp, ref, target)
    c = {q: max(FLOOR, units(getattr(lo, q), getattr(ref, q), S[q])) for q in S}
    return ref, lo, S, c


def units(got, ref, S) -> float:
    """max |got - ref| in units of 2^-24 S over the elements; an element of scale 0 must be exact."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    if np.any(d[S == 0] != 0):
        return math.inf
    nz = S > 0
    return float(np.max(d[nz] / (U24 * S[nz]))) if nz.any() else 0.0


# ---------------------------------------------------------------------------- reachable moments
def moment_ratio_bound(b1: float, b2: float) -> float:
    """C with |mu_t| <= C sqrt(nu_t) for every gradient sequence and t (Cauchy-Schwarz over the two
    geometric sums): engine.cpp adam_step_bound_of without the bias-correction ratio and its 1.25."""
    return (1 - b1) / math.sqrt((1 - b2) * (1 - b1 * b1 / b2))


def reachable_moments(g_ref, hp: Hyper, seed: int, steps: int = 4):
    """(mu0, nu0) float32 as `steps` Adam steps from zero leave them, over the gradients
    g_ref * N(0, 1) elementwise.

    Reachability matters.  The split2h engine sizes the exponent of the weight planes an update writes
    from max |p| before it plus adam_step_bound() lr (engine.cpp adam_step_bound_of), a bound on |p' - p|
    that holds for moments produced by ANY gradient sequence at any count >= 1, because then
    |mu| <= C sqrt(nu).  It does not hold for arbitrary (mu, nu) pairs (mu = 1, nu = 1e-12 moves a weight
    by 1e6 lr), so a test that loads random moments can overflow the planes of a correct engine."""
    rng = np.random.default_rng(seed)
    g_ref = np.asarray(g_ref, np.float64)
    mu, nu = np.zeros_like(g_ref), np.zeros_like(g_ref)
    for _ in range(steps):
        g = g_ref * rng.standard_normal(g_ref.shape)
        mu = (1 - hp.b1) * g + hp.b1 * mu
        nu = (1 - hp.b2) * g * g + hp.b2 * nu
    return mu.astype(np.float32), nu.astype(np.float32)
