"""Float64 CAGrad training step for the tests (a helper, not a test module).

One ``MTSAC._update_inner`` with ``CAGradConfig`` on both optimizers: the split-loss step of
tests/pcgrad_oracle.py (its per-task gradient functions are used as they are) with the surgery replaced
by the reference's literal CAGrad statement on the gradients themselves
(``mtrl_amd.cagrad.cagrad_direct``: rows clipped to norm 1, the Gram of the clipped rows, the objective
differentiated by torch.autograd in float64), then clip_by_global_norm, Adam, Polyak as before.
"""

from __future__ import annotations

import numpy as np

import pcgrad_oracle as po
from mtrl_amd.cagrad import LOG_KEYS, cagrad_direct
from oracle import conflict as oc
from oracle import mtsac as om

CA_KEYS = LOG_KEYS


def matrix_families(T, P, seed):
    """The five families the degeneracy of the reference's search was checked on: random rows with norms
    on both sides of 1, half of the rows conflicting with the other half, rows cancelling exactly in
    pairs, tiny, zero."""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((T, P)) * rng.uniform(0.02, 0.5, (T, 1))
    H = R.copy()
    H[T // 2:] = -0.7 * R[:T - T // 2] + 0.03 * rng.standard_normal((T - T // 2, P))
    C = R.copy()
    C[1::2] = -C[0::2][:len(C[1::2])]
    if T % 2:
        C[-1] = 0.0
    return {"random": R, "half_conflicting": H, "cancelling": C, "tiny": R * 1e-9, "zero": np.zeros((T, P))}


def update(cfg, state, batch, eps_next, eps_cur, cosine_sim_logs=False, **hyper):
    """(new_state, logs): logs = the ten MTSAC logs + the ten CAGradState entries (task_weights arrays)."""
    assert not cfg.use_task_weights
    s = state.copy()
    batch = [np.asarray(b, np.float64) for b in batch]
    obs = batch[0]
    T, B = cfg.num_tasks, obs.shape[0]
    # critic
    qf_values, qf_loss = po._critic_losses(cfg, s, batch, eps_next)
    Gc, _ = oc.task_grads(cfg, s, batch, eps_next, eps_cur)
    gc, logs_c = cagrad_direct(Gc, cosine_sim_logs=cosine_sim_logs, **hyper)
    s.critic = om.adam_step(s.critic, om.clip_by_global_norm(gc, cfg.critic_max_grad_norm), s.critic_opt,
                            cfg.critic_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    s.critic_target = cfg.tau * s.critic + (1.0 - cfg.tau) * s.critic_target
    # actor through the updated critic
    Ga, loss_t, exp_t, logpi = po._actor_task_grads(cfg, s, batch, eps_cur)
    ga, logs_a = cagrad_direct(Ga, cosine_sim_logs=cosine_sim_logs, **hyper)
    s.actor = om.adam_step(s.actor, om.clip_by_global_norm(ga, cfg.actor_max_grad_norm), s.actor_opt,
                           cfg.actor_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    # temperature (mtsac.py:713-731)
    task_ids = obs[:, -T:]
    lp = logpi.reshape(-1, 1) + cfg.target_entropy
    alpha_loss = (-(task_ids @ s.log_alpha.reshape(-1, 1)) * lp).mean()
    g_la = om.clip_by_global_norm((-(task_ids * lp)).sum(axis=0) / B, cfg.alpha_max_grad_norm)
    s.log_alpha = om.adam_step(s.log_alpha, g_la, s.alpha_opt, cfg.alpha_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    logs = {
        "losses/qf_values": qf_values,
        "losses/qf_loss": qf_loss,
        "metrics/critic_grad_magnitude": logs_c["grad_magnitude"],
        "metrics/critic_params_norm": om.global_norm(s.critic),
        "losses/actor_loss": float(loss_t.mean()),
        "metrics/actor_grad_magnitude": logs_a["grad_magnitude"],
        "metrics/actor_params_norm": om.global_norm(s.actor),
        "metrics/explore_loss": float(exp_t.mean()),
        "losses/alpha_loss": float(alpha_loss),
        "alpha": float(np.exp(s.log_alpha).sum()),
    }
    for net, lg in (("critic", logs_c), ("actor", logs_a)):
        for k in CA_KEYS:
            logs[f"metrics/{net}_{k}"] = lg[k]
    return s, logs
