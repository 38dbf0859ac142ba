"""Float64 PCGrad training step for the tests (a helper, not a test module).

One ``MTSAC._update_inner`` with ``PCGradConfig`` on both optimizers, assembled from the oracle's
primitives (oracle/mtsac.py, oracle/conflict.py):

  1. per-task critic gradients (split losses, mtsac.py:513-598: the "next" actions sampled from
     pi(.|s) of the OBSERVATIONS, scored by the target critic at s');
  2. the surgery, the reference's literal sequential projection (mtrl/optim/pcgrad.py:56-95) on the rows
     taken in the order ``perm``;
  3. clip_by_global_norm, Adam, Polyak;
  4. per-task actor gradients through the UPDATED critic, each task's loss with the explore term
     ``- mean((a_data - a)^2)`` (mtsac.py:668-673, the default ``_explore=True`` of the split call);
  5. surgery, clip, Adam;
  6. temperature.

Noise is injected per row ([B][A]); the reference's vmap hands every task the same key, which a caller
reproduces by repeating one (n, A) draw over the tasks.
"""

from __future__ import annotations

import numpy as np

from oracle import conflict as oc
from oracle import mtsac as om

PC_KEYS = ("n_grad_conflicts", "avg_grad_magnitude", "avg_grad_magnitude_before_surgery",
           "avg_cosine_similarity", "avg_cosine_similarity_diff")


def _avg_cos(M):
    T = M.shape[0]
    nrm = np.linalg.norm(M, axis=1)
    cos = (M @ M.T) / (nrm[:, None] * nrm[None, :] + 1e-8)
    return float(np.triu(cos, k=1).sum() / (T * (T - 1) / 2 + 1e-8))


def surgery(M, perm, cosine_sim_logs=False):
    """(mean_i g_i^pc, PCGradState logs, margin): the literal projection on M[perm].  margin = the
    smallest |cos(g_i^pc, g_j)| over every decision with j != i (how far each ``proj < 0`` test is
    from flipping under rounding)."""
    Mp = np.asarray(M, np.float64)[np.asarray(perm)]
    T = Mp.shape[0]
    final = np.empty_like(Mp)
    total, margin = 0, np.inf
    for i in range(T):
        g = Mp[i].copy()
        for j in range(T):
            dot = np.dot(g, Mp[j])
            proj = dot / ((Mp[j] ** 2).sum() + 1e-8)
            if j != i:
                margin = min(margin, abs(dot) / (np.linalg.norm(g) * np.linalg.norm(Mp[j])))
            g = g - min(proj, 0.0) * Mp[j]
            total += int(proj < 0)
        final[i] = g
    logs = {
        "n_grad_conflicts": total / 2,
        "avg_grad_magnitude": float(np.linalg.norm(final, axis=1).mean()),
        "avg_grad_magnitude_before_surgery": float(np.linalg.norm(Mp, axis=1).mean()),
        "avg_cosine_similarity": float("nan"),
        "avg_cosine_similarity_diff": float("nan"),
    }
    if cosine_sim_logs:
        before = _avg_cos(Mp)
        logs["avg_cosine_similarity"] = before
        logs["avg_cosine_similarity_diff"] = before - _avg_cos(final)
    return final.mean(axis=0), logs, float(margin)


def _actor_task_grads(cfg, state, batch, eps_cur):
    """Per-task actor gradients with the explore term; (G [T][P], loss_t [T], explore_t [T], logpi [B])."""
    obs, act = np.asarray(batch[0], np.float64), np.asarray(batch[1], np.float64)
    T, A, C = cfg.num_tasks, cfg.action_dim, cfg.num_critics
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc = om.unflatten(state.actor, ash), om.unflatten(state.critic, csh)
    task_ids = obs[:, -T:]
    tasks = np.argmax(task_ids, axis=1)
    alpha = np.exp(task_ids @ state.log_alpha.reshape(-1, 1))
    G = np.zeros((T, om.num_params(ash)))
    loss_t, exp_t = np.zeros(T), np.zeros(T)
    logpi = np.zeros(obs.shape[0])
    for t in range(T):
        r = np.flatnonzero(tasks == t)
        n = r.size
        o, a_d, al = obs[r], act[r], alpha[r]
        out, hs_a, t_a = om.mh_forward(pa, o, cfg.actor_depth, T)
        a_c, lp_c, pcache = om.tanh_normal_sample(out, eps_cur[r], cfg)
        logpi[r] = lp_c
        q_pi, caches_pi = om.critic_forward(pc, np.concatenate([a_c, o], axis=1), cfg)
        exp_t[t] = np.mean((a_d - a_c) ** 2)
        loss_t[t] = (al * lp_c.reshape(-1, 1) - q_pi.min(axis=0)).mean() - exp_t[t]
        g_logpi = al.reshape(-1) / n
        dq_pi = om.min_grad(q_pi) * (-np.ones((n, 1)) / n)[None]
        g_a = 2.0 * (a_d - a_c) / (n * A)  # d(-mean((a_d - a)^2)) / da
        for k in range(C):
            hs, tt = caches_pi[k]
            _, dx = om.mh_backward(om.ens_slice(pc, k), hs, tt, dq_pi[k], cfg.critic_depth, need_dx=True)
            g_a = g_a + dx[:, :A]
        dout = om.tanh_normal_backward(pcache, g_a, g_logpi, cfg)
        ga, _ = om.mh_backward(pa, hs_a, t_a, dout, cfg.actor_depth)
        G[t] = om.flatten(ga, ash)
    return G, loss_t, exp_t, logpi


def _critic_losses(cfg, state, batch, eps_next):
    """(qf_values, qf_loss) of the split critic loss: means over tasks of the per-task means."""
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
    return float(q.mean()), float(((q - y[None]) ** 2).mean())


def update(cfg, state, batch, eps_next, eps_cur, perm_critic, perm_actor, cosine_sim_logs=False):
    """(new_state, logs, margins): logs = the ten MTSAC logs + the ten PCGradState entries;
    margins = (critic, actor) decision margins of ``surgery``."""
    assert not cfg.use_task_weights
    s = state.copy()
    batch = [np.asarray(b, np.float64) for b in batch]
    obs = batch[0]
    T, B = cfg.num_tasks, obs.shape[0]
    # critic
    qf_values, qf_loss = _critic_losses(cfg, s, batch, eps_next)
    Gc, _ = oc.task_grads(cfg, s, batch, eps_next, eps_cur)
    gc, logs_c, margin_c = surgery(Gc, perm_critic, cosine_sim_logs)
    critic_gnorm = om.global_norm(Gc.mean(axis=0))
    s.critic = om.adam_step(s.critic, om.clip_by_global_norm(gc, cfg.critic_max_grad_norm), s.critic_opt,
                            cfg.critic_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    s.critic_target = cfg.tau * s.critic + (1.0 - cfg.tau) * s.critic_target
    # actor through the updated critic
    Ga, loss_t, exp_t, logpi = _actor_task_grads(cfg, s, batch, eps_cur)
    ga, logs_a, margin_a = surgery(Ga, perm_actor, cosine_sim_logs)
    actor_gnorm = om.global_norm(Ga.mean(axis=0))
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
        "metrics/critic_grad_magnitude": critic_gnorm,
        "metrics/critic_params_norm": om.global_norm(s.critic),
        "losses/actor_loss": float(loss_t.mean()),
        "metrics/actor_grad_magnitude": actor_gnorm,
        "metrics/actor_params_norm": om.global_norm(s.actor),
        "metrics/explore_loss": float(exp_t.mean()),
        "losses/alpha_loss": float(alpha_loss),
        "alpha": float(np.exp(s.log_alpha).sum()),
    }
    for net, lg in (("critic", logs_c), ("actor", logs_a)):
        for k in PC_KEYS:
            logs[f"metrics/{net}_{k}"] = lg[k]
    return s, logs, (margin_c, margin_a)


def head_init_state(cfg, seed, head_bound=1.0):
    """An oracle state whose head leaves are U(+-head_bound) (with the default +-1e-3 / +-3e-3 heads the
    per-task gradients are orthogonal to ~1e-6 and every projection decision would hinge on rounding),
    rounded through float32."""
    rng = np.random.default_rng(seed)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    a = om.flatten(om.init_network(rng, ash, head_bound), ash)
    c = om.flatten(om.init_network(rng, csh, head_bound), csh)
    la = np.full(cfg.num_tasks, np.log(cfg.initial_temperature))
    st = om.MTSACState(a, c, c.copy(), la, om.AdamState.zeros(a.size, np.float64),
                       om.AdamState.zeros(c.size, np.float64), om.AdamState.zeros(la.size, np.float64))
    for k in ("actor", "critic", "critic_target", "log_alpha"):
        setattr(st, k, getattr(st, k).astype(np.float32).astype(np.float64))
    return st
