"""GradNorm (mtrl/optim/gradnorm.py, GradNormConfig of mtrl/config/optim.py) in Gram form, numpy float64.

The optimizer's effect on the per-task gradients ``M`` [T][P] is a vector of T combine weights computed
from the diagonal of ``G = M M^T``, the per-task loss values and a state carried from step to step
(DESIGN.md section 12):

    per-task clip:  s_t = min(1, 1 / (|g_t| + 1e-8)) when GradNormConfig.max_grad_norm is truthy (the bound
                    is 1.0, clip_per_task_grads' default, whatever max_grad_norm is), else s_t = 1
    latch:          L0_t <- L_t where isinf(L0_t)
    rates:          imp_t = L_t / (L0_t + 1e-12),  r_t = imp_t / (mean imp + 1e-12)
    gradnorm loss:  n_t = s_t sqrt(G_tt) (reference form) or |w_t| s_t sqrt(G_tt) (weighted form),
                    d_t = n_t - mean(n) r_t^asymmetry,  loss = sum_t |d_t|
    weight step:    grad = d loss / d w, [clip_by_global_norm], Adam on the T weights, w <- w + update
                    (float32), w <- (w / sum w) * T (float32)
    combine:        update = sum_t w_t s_t g_t   (a SUM over the tasks, not a mean)

In the reference form the loss does not depend on the weights (gradnorm.py:130-141; the version that
multiplies by the weights is commented out, :115-128), so ``grad`` is exactly zero whatever the loss
value is, NaN included: the inner Adam's count advances, ``mu``, ``nu`` and the update stay 0 and the
weights stay the normalised ``initial_weights``.  ``weighted_norms=True`` is the commented-out block
(the paper's form, targets not held constant, as there); GradNormConfig never sets it.  A negative
``r_t`` (actor losses are negative whenever their first value was positive, and the other way round)
gives ``r_t ** asymmetry`` = NaN as ``jnp.power`` does; it propagates into ``gradnorm_loss`` in both
forms and, in the weighted form, into the weights.  It is not guarded.

The state is held in float32 (the reference's dtype, and the device's); the arithmetic is float64 with
the final renormalisation in float32, in the reference's order.  ``gradnorm_from_gram`` is the host
statement of the device solve (csrc/gradnorm.hip); ``gradnorm_direct`` is the reference's literal
statement on the gradients themselves, the gradient with respect to the weights taken by
``torch.autograd`` in float64.
"""

from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

LOG_KEYS = ("task_weights", "original_losses")  # GradNormState fields logged per network (mtsac.py:1224-1239)
ADAM_B1, ADAM_B2 = 0.9, 0.999  # optax.adam's defaults, which OptimizerConfig.spawn leaves alone


@dataclass(frozen=True)
class GradNormState:
    """gradnorm.py:34-37 with the inner optimizer's ScaleByAdamState spelled out."""

    task_weights: np.ndarray     # [T] float32
    original_losses: np.ndarray  # [T] float32, +inf until latched
    count: int                   # inner Adam
    mu: np.ndarray               # [T] float32
    nu: np.ndarray               # [T] float32


def renormalise(w, T: int) -> np.ndarray:
    """(w / sum w) * T in float32 (gradnorm.py:79, 149)."""
    w = np.asarray(w, np.float32)
    return (w / w.sum(dtype=np.float32)) * np.float32(T)


def gradnorm_init(T: int, initial_weights=None) -> GradNormState:
    """gradnorm.py:70-84: the inner optimizer is initialised (zeros), then the weights are normalised."""
    w = np.ones(T, np.float32) if initial_weights is None else np.array(initial_weights, np.float32).reshape(T)
    return GradNormState(renormalise(w, T), np.full(T, np.inf, np.float32), 0, np.zeros(T, np.float32),
                         np.zeros(T, np.float32))


def _sign(x):
    return np.sign(x)  # sign(0) = 0, NaN stays NaN


def _rates(task_losses, state: GradNormState):
    L = np.asarray(task_losses, np.float64).reshape(-1)
    L0 = state.original_losses.astype(np.float64)
    L0 = np.where(np.isinf(L0), L, L0)
    with np.errstate(all="ignore"):
        imp = L / (L0 + 1e-12)
        r = imp / (imp.mean() + 1e-12)
    return L0, r


def _weights_step(grad, state: GradNormState, L0, inner_lr, inner_eps, inner_max_grad_norm):
    """optax.chain([clip_by_global_norm], adam) on the task weights, apply_updates, renormalise."""
    T = grad.shape[0]
    g = np.asarray(grad, np.float64)
    with np.errstate(all="ignore"):
        if inner_max_grad_norm is not None:
            gn = np.sqrt((g * g).sum())
            g = g if gn < inner_max_grad_norm else (g / gn) * inner_max_grad_norm
        count = state.count + 1
        mu = ADAM_B1 * state.mu.astype(np.float64) + (1.0 - ADAM_B1) * g
        nu = ADAM_B2 * state.nu.astype(np.float64) + (1.0 - ADAM_B2) * g * g
        upd = -inner_lr * (mu / (1.0 - ADAM_B1 ** count)) / (np.sqrt(nu / (1.0 - ADAM_B2 ** count)) + inner_eps)
        w = renormalise((state.task_weights.astype(np.float64) + upd).astype(np.float32), T)
    return replace(state, task_weights=w, original_losses=L0.astype(np.float32), count=count,
                   mu=mu.astype(np.float32), nu=nu.astype(np.float32))


def weighted_grad(w, nt, r, asymmetry):
    """(loss, d, avg, grad) of the weighted form: N_t = |w_t| nt_t, d_t = N_t - mean(N) r_t^a,
    grad_i = sign(w_i) nt_i (sign(d_i) - (1/T) sum_j sign(d_j) r_j^a)."""
    with np.errstate(all="ignore"):
        ra = np.power(r, asymmetry)
        N = np.abs(w) * nt
        avg = N.mean()
        d = N - avg * ra
        sg = _sign(d)
        grad = _sign(w) * nt * (sg - (sg * ra).sum() / w.shape[0])
    return float(np.abs(d).sum()), d, float(avg), grad


def gradnorm_from_gram(gram, task_losses, state: GradNormState, *, asymmetry: float = 0.12,
                       per_task_clip: bool = True, inner_lr: float = 3e-4, inner_eps: float = 1e-5,
                       inner_max_grad_norm: float | None = 1.0, weighted_norms: bool = False):
    """(w_combine [T] on the raw rows, new_state, logs) from the Gram matrix of the raw task gradients.

    ``logs``: task_weights, original_losses (the new state's), ``grad_magnitude`` = |mean_t g_t| of the raw
    rows, ``gradnorm_loss`` and ``sign_margin`` = min_t |d_t| / mean(n): how far every sign decision of
    the loss is from flipping under rounding; also ``rates`` (r_t), ``weights_grad`` (the gradient the inner
    optimizer saw) and ``combine_weights``.  A negative r_t makes gradnorm_loss NaN (see the module)."""
    G = np.asarray(gram, np.float64)
    T = G.shape[0]
    nrm = np.sqrt(np.maximum(np.diag(G), 0.0))
    s = np.minimum(1.0, 1.0 / (nrm + 1e-8)) if per_task_clip else np.ones(T)
    nt = s * nrm
    L0, r = _rates(task_losses, state)
    w_old = state.task_weights.astype(np.float64)
    loss, d, avg, grad = weighted_grad(w_old if weighted_norms else np.ones(T), nt, r, asymmetry)
    if not weighted_norms:
        grad = np.zeros(T)  # the loss does not touch the weights
    new = _weights_step(grad, state, L0, inner_lr, inner_eps, inner_max_grad_norm)
    with np.errstate(all="ignore"):
        margin = float(np.abs(d).min() / avg)
    logs = {"task_weights": new.task_weights, "original_losses": new.original_losses,
            "grad_magnitude": float(np.sqrt(max(G.sum(), 0.0)) / T), "gradnorm_loss": loss,
            "sign_margin": margin, "rates": r, "weights_grad": grad}
    logs["combine_weights"] = new.task_weights.astype(np.float64) * s
    return logs["combine_weights"], new, logs


def gradnorm_direct(M, task_losses, state: GradNormState, *, asymmetry: float = 0.12, per_task_clip: bool = True,
                    inner_lr: float = 3e-4, inner_eps: float = 1e-5, inner_max_grad_norm: float | None = 1.0,
                    weighted_norms: bool = False):
    """The reference's statement on the gradients themselves (gradnorm.py:86-161): rows clipped, the loss
    on the row norms differentiated with respect to the task weights by torch.autograd in float64 -- in the
    reference form through a loss that does not touch them (``allow_unused``, turned into zeros, as
    jax.grad gives): (update [P], new_state, logs)."""
    import torch

    M = np.asarray(M, np.float64)
    T = M.shape[0]
    nrm = np.linalg.norm(M, axis=1)
    s = np.minimum(1.0, 1.0 / (nrm + 1e-8)) if per_task_clip else np.ones(T)
    Mc = M * s[:, None]
    L0, r = _rates(task_losses, state)
    wt = torch.tensor(state.task_weights.astype(np.float64), requires_grad=True)
    Mc_t = torch.tensor(Mc, requires_grad=True)  # a leaf, so that the reference form's loss has a graph at all
    r_t = torch.from_numpy(r)
    norms = torch.linalg.norm(wt[:, None] * Mc_t, dim=1) if weighted_norms else torch.linalg.norm(Mc_t, dim=1)
    avg = norms.mean()
    d = norms - avg * r_t ** asymmetry
    loss = d.abs().sum()
    (g,) = torch.autograd.grad(loss, wt, allow_unused=True)
    grad = np.zeros(T) if g is None else g.numpy()
    new = _weights_step(grad, state, L0, inner_lr, inner_eps, inner_max_grad_norm)
    with np.errstate(all="ignore"):
        margin = float(np.abs(d.detach().numpy()).min() / avg.item())
    logs = {"task_weights": new.task_weights, "original_losses": new.original_losses,
            "grad_magnitude": float(np.linalg.norm(M.mean(axis=0))), "gradnorm_loss": loss.item(),
            "sign_margin": margin, "rates": r, "weights_grad": grad,
            "combine_weights": new.task_weights.astype(np.float64) * s}
    return new.task_weights.astype(np.float64) @ Mc, new, logs
