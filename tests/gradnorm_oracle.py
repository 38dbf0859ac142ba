"""Float64 GradNorm training step for the tests (a helper, not a test module).

One ``MTSAC._update_inner`` with ``GradNormConfig`` on both optimizers: the split-loss step of
tests/pcgrad_oracle.py (its per-task gradient functions are used as they are; the per-task critic loss
VALUES are computed here, ``_critic_losses`` returning their means only) with the surgery replaced by the
reference's literal GradNorm statement on the gradients themselves (``mtrl_amd.gradnorm.gradnorm_direct``:
rows clipped to norm 1, the loss on the row norms differentiated with respect to the task weights by
torch.autograd in float64), then clip_by_global_norm, Adam, Polyak as before.  The two GradNormStates are
threaded through the steps by the caller.
"""

from __future__ import annotations

import numpy as np

import pcgrad_oracle as po
from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_init
from oracle import conflict as oc
from oracle import mtsac as om


def init(T, initial_weights=None):
    """(critic state, actor state)."""
    return gradnorm_init(T, initial_weights), gradnorm_init(T, initial_weights)


def critic_task_losses(cfg, state, batch, eps_next):
    """(qf_values, per-task critic loss values [T]): task t's mean over its rows and the ensemble of the
    squared TD errors (mtsac.py:563-566 under the vmap of :569-580)."""
    obs, act, nobs, dones, rew = [np.asarray(b, np.float64) for b in batch]
    T = cfg.num_tasks
    B = obs.shape[0]
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc, pt = om.unflatten(state.actor, ash), om.unflatten(state.critic, csh), om.unflatten(state.critic_target, csh)
    alpha = np.exp(obs[:, -T:] @ state.log_alpha.reshape(-1, 1))
    out, _, _ = om.mh_forward(pa, obs, cfg.actor_depth, T)
    a_n, lp_n, _ = om.tanh_normal_sample(out, eps_next, cfg)
    q_t, _ = om.critic_forward(pt, np.concatenate([a_n, nobs], axis=1), cfg)
    y = rew.reshape(B, 1) + (1.0 - dones.reshape(B, 1)) * cfg.gamma * (q_t.min(axis=0) - alpha * lp_n.reshape(-1, 1))
    q, _ = om.critic_forward(pc, np.concatenate([act, obs], axis=1), cfg)
    if cfg.clip:
        y, q = np.clip(y, -5000, 5000), np.clip(q, -5000, 5000)
    sq = ((q - y[None]) ** 2).reshape(q.shape[0], B)
    tasks = np.argmax(obs[:, -T:], axis=1)
    return float(q.mean()), np.array([sq[:, tasks == t].mean() for t in range(T)])


def update(cfg, state, gn, batch, eps_next, eps_cur, require_margin=None, **hyper):
    """(new_state, (new critic GradNormState, new actor GradNormState), logs).  ``hyper``: gradnorm_direct's
    keywords, for both networks.  ``require_margin``: assert r > 0 and sign_margin >= it at both solves
    (the weighted form's condition for a comparison against fp32 arithmetic)."""
    assert not cfg.use_task_weights
    s = state.copy()
    batch = [np.asarray(b, np.float64) for b in batch]
    obs = batch[0]
    T, B = cfg.num_tasks, obs.shape[0]
    # critic
    qf_values, Lc = critic_task_losses(cfg, s, batch, eps_next)
    assert abs(Lc.mean() - po._critic_losses(cfg, s, batch, eps_next)[1]) <= 1e-12 * abs(Lc.mean())
    Gc, _ = oc.task_grads(cfg, s, batch, eps_next, eps_cur)
    gc, gn_c, logs_c = gradnorm_direct(Gc, Lc, gn[0], **hyper)
    s.critic = om.adam_step(s.critic, om.clip_by_global_norm(gc, cfg.critic_max_grad_norm), s.critic_opt,
                            cfg.critic_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    s.critic_target = cfg.tau * s.critic + (1.0 - cfg.tau) * s.critic_target
    # actor through the updated critic
    Ga, loss_t, exp_t, logpi = po._actor_task_grads(cfg, s, batch, eps_cur)
    ga, gn_a, logs_a = gradnorm_direct(Ga, loss_t, gn[1], **hyper)
    s.actor = om.adam_step(s.actor, om.clip_by_global_norm(ga, cfg.actor_max_grad_norm), s.actor_opt,
                           cfg.actor_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    if require_margin is not None:
        for lg in (logs_c, logs_a):
            assert np.all(lg["rates"] > 0.0), lg["rates"]
            assert lg["sign_margin"] >= require_margin, lg["sign_margin"]
    # temperature (mtsac.py:713-731)
    task_ids = obs[:, -T:]
    lp = logpi.reshape(-1, 1) + cfg.target_entropy
    alpha_loss = (-(task_ids @ s.log_alpha.reshape(-1, 1)) * lp).mean()
    g_la = om.clip_by_global_norm((-(task_ids * lp)).sum(axis=0) / B, cfg.alpha_max_grad_norm)
    s.log_alpha = om.adam_step(s.log_alpha, g_la, s.alpha_opt, cfg.alpha_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    logs = {
        "losses/qf_values": qf_values,
        "losses/qf_loss": float(Lc.mean()),
        "metrics/critic_grad_magnitude": logs_c["grad_magnitude"],
        "metrics/critic_params_norm": om.global_norm(s.critic),
        "losses/actor_loss": float(loss_t.mean()),
        "metrics/actor_grad_magnitude": logs_a["grad_magnitude"],
        "metrics/actor_params_norm": om.global_norm(s.actor),
        "metrics/explore_loss": float(exp_t.mean()),
        "losses/alpha_loss": float(alpha_loss),
        "alpha": float(np.exp(s.log_alpha).sum()),
        "critic_task_losses": Lc,
        "actor_task_losses": loss_t,
    }
    for net, lg in (("critic", logs_c), ("actor", logs_a)):
        for k in ("task_weights", "original_losses", "gradnorm_loss", "sign_margin"):
            logs[f"metrics/{net}_{k}"] = lg[k]
    return s, (gn_c, gn_a), logs
