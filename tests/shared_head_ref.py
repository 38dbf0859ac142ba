"""Float64 MTSAC step of the shared-head (Vanilla) network for the tests (a helper, not a test module).

The reference's ``VanillaNetworkConfig`` builds ``VanillaNetwork`` -> ``MLP`` (mtrl/nn/base.py:11-89): ``depth``
Dense+ReLU layers ``layer_0 .. layer_{D-1}`` and ONE Dense head ``layer_D`` for all tasks.  A shared head is
T tied heads: the forward and backward run on the oracle's multi-head pieces (``mh_forward``, ``mh_backward``,
``critic_forward``, ``tanh_normal_*``, ``min_grad``) with the head broadcast over the tasks (``tie``), and the
head gradient is the SUM of the T blocks (``untie_grad``); clip, Adam and Polyak then run on the Vanilla-ordered
vector.  ``oracle.update`` itself cannot serve as the step: its global norm over the tied copies would count
the head T times.

Vectors are in the flax leaf order of the Vanilla tree: layer_0/bias, layer_0/kernel, ..., layer_D/bias,
layer_D/kernel (the head LAST; critic leaves with the leading ensemble axis) -- the order of
``mtsac_set_params`` on an engine created with MTSAC_NET_SHARED_HEAD.

Per-task gradients (``task_grads``, ``actor_task_grads``): the split losses of the task-gradient pass as
oracle/conflict.py and tests/pcgrad_oracle.py state them, run on the tied heads; row t's head gradient is
block t (the other blocks are zero), which ``untie_rows`` moves to the head's columns.
"""

from __future__ import annotations

import numpy as np

import pcgrad_oracle as po
from oracle import conflict as oc
from oracle import mtsac as om


# ------------------------------------------------------------------ leaves
def vanilla_shapes(in_dim: int, width: int, depth: int, head_dim: int, ens: int | None):
    pre = () if ens is None else (ens,)
    shapes, fan = [], in_dim
    for i in range(depth):
        shapes += [(f"b{i}", pre + (width,)), (f"W{i}", pre + (fan, width))]
        fan = width
    return shapes + [("head_b", pre + (head_dim,)), ("head_W", pre + (width, head_dim))]


def actor_shapes(cfg):
    return vanilla_shapes(cfg.actor_in, cfg.actor_width, cfg.actor_depth, 2 * cfg.action_dim, None)


def critic_shapes(cfg):
    return vanilla_shapes(cfg.critic_in, cfg.critic_width, cfg.critic_depth, 1, cfg.num_critics)


def param_count(in_dim, width, depth, head_dim, ens=1):
    """in W + W + (D - 1)(W^2 + W) + W hd + hd per member."""
    return ens * (in_dim * width + width + (depth - 1) * (width * width + width) + width * head_dim + head_dim)


def tie(flat_v, shapes_v, shapes_mh, T):
    """Vanilla flat vector -> multi-head flat vector with the head broadcast to T tied heads."""
    p = om.unflatten(np.asarray(flat_v), shapes_v)
    ens = len(p["b0"].shape) == 2
    q = dict(p)
    for k in ("head_b", "head_W"):
        q[k] = np.repeat(np.expand_dims(p[k], 1 if ens else 0), T, axis=1 if ens else 0)
    return om.flatten(q, shapes_mh)


def untie_grad(flat_mh, shapes_v, shapes_mh):
    """Multi-head gradient -> Vanilla gradient: the head blocks summed over the tasks."""
    g = om.unflatten(np.asarray(flat_mh), shapes_mh)
    ens = len(g["b0"].shape) == 2
    q = dict(g)
    for k in ("head_b", "head_W"):
        q[k] = g[k].sum(axis=1 if ens else 0)
    return om.flatten(q, shapes_v)


def untie_rows(G_mh, shapes_v, shapes_mh):
    return np.stack([untie_grad(r, shapes_v, shapes_mh) for r in G_mh])


def tied_state(cfg, st):
    """The multi-head oracle state holding T tied copies of the shared heads (parameters only)."""
    T = cfg.num_tasks
    a = tie(st.actor, actor_shapes(cfg), om.actor_leaf_shapes(cfg), T)
    c = tie(st.critic, critic_shapes(cfg), om.critic_leaf_shapes(cfg), T)
    ct = tie(st.critic_target, critic_shapes(cfg), om.critic_leaf_shapes(cfg), T)
    z = lambda n: om.AdamState.zeros(n, np.float64)  # noqa: E731
    return om.MTSACState(a, c, ct, st.log_alpha.copy(), z(a.size), z(c.size), z(st.log_alpha.size))


def initialize(cfg, seed=1, head_bound=None):
    """Vanilla-ordered state: he_uniform trunk, zero biases, head kernel and bias uniform(1e-3) actor / uniform(3e-3)
    critic (``head_bound`` overrides both), rounded through float32."""
    rng = np.random.default_rng(seed)
    ash, csh = actor_shapes(cfg), critic_shapes(cfg)
    a = om.flatten(om.init_network(rng, ash, head_bound or 1e-3), ash)
    c = om.flatten(om.init_network(rng, csh, head_bound or 3e-3), csh)
    la = np.full(cfg.num_tasks, np.log(cfg.initial_temperature))
    st = om.MTSACState(a, c, c.copy(), la, om.AdamState.zeros(a.size, np.float64),
                       om.AdamState.zeros(c.size, np.float64), om.AdamState.zeros(la.size, np.float64))
    for k in ("actor", "critic", "critic_target", "log_alpha"):
        setattr(st, k, getattr(st, k).astype(np.float32).astype(np.float64))
    return st


# ------------------------------------------------------------------ losses and gradients on the tied heads
def critic_loss_grad(cfg, st, batch, eps_next, skip_task=None):
    """(qf_loss, qf_values, Vanilla-ordered gradient) of the critic loss (mtsac.py:513-566).  skip_task: a seeded
    ERROR for the bars' own test -- that task's block is left out of the head gradient's sum."""
    obs, act, nobs, dones, rew = [np.asarray(b, np.float64) for b in batch]
    T, C, B = cfg.num_tasks, cfg.num_critics, obs.shape[0]
    ts = tied_state(cfg, st)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc, pt = om.unflatten(ts.actor, ash), om.unflatten(ts.critic, csh), om.unflatten(ts.critic_target, csh)
    task_ids = obs[:, -T:]
    alpha = np.exp(task_ids @ st.log_alpha.reshape(-1, 1))
    tw = _task_weights(cfg, st, task_ids)
    out_n, _, _ = om.mh_forward(pa, nobs, cfg.actor_depth, T)
    a_n, logpi_n, _ = om.tanh_normal_sample(out_n, eps_next, cfg)
    q_t, _ = om.critic_forward(pt, np.concatenate([a_n, nobs], axis=1), cfg)
    y = rew.reshape(B, 1) + (1.0 - dones.reshape(B, 1)) * cfg.gamma * (q_t.min(axis=0) - alpha * logpi_n.reshape(-1, 1))
    q, caches = om.critic_forward(pc, np.concatenate([act, obs], axis=1), cfg)
    if cfg.clip:
        y, qc, dclip = np.clip(y, -5000, 5000), np.clip(q, -5000, 5000), om.clip_grad_factor(q, -5000.0, 5000.0)
    else:
        qc, dclip = q, np.ones_like(q)
    diff = qc - y[None]
    w = tw[None] if tw is not None else 1.0
    dq = (w * 2.0 * diff / (C * B)) * dclip
    gc = {}
    for k in range(C):
        hs, t = caches[k]
        g, _ = om.mh_backward(om.ens_slice(pc, k), hs, t, dq[k], cfg.critic_depth)
        for n, v in g.items():
            gc.setdefault(n, []).append(v)
    gc = {n: np.stack(v) for n, v in gc.items()}
    if skip_task is not None:
        gc["head_W"][:, skip_task] = 0.0
        gc["head_b"][:, skip_task] = 0.0
    return float((w * diff * diff).mean()), float(qc.mean()), untie_grad(om.flatten(gc, csh), critic_shapes(cfg), csh)


def _task_weights(cfg, st, task_ids):
    if not cfg.use_task_weights:
        return None
    e = np.exp(-st.log_alpha - np.max(-st.log_alpha))
    return (task_ids @ (e / e.sum()).reshape(-1, 1)) * cfg.num_tasks


def actor_loss_grad(cfg, st, batch, eps_cur, skip_task=None):
    """(actor_loss, Vanilla-ordered gradient, logpi [B]) of the actor loss through st.critic (mtsac.py:623-691)."""
    obs = np.asarray(batch[0], np.float64)
    T, A, C, B = cfg.num_tasks, cfg.action_dim, cfg.num_critics, obs.shape[0]
    ts = tied_state(cfg, st)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc = om.unflatten(ts.actor, ash), om.unflatten(ts.critic, csh)
    task_ids = obs[:, -T:]
    alpha = np.exp(task_ids @ st.log_alpha.reshape(-1, 1))
    tw = _task_weights(cfg, st, task_ids)
    out_c, hs_a, t_a = om.mh_forward(pa, obs, cfg.actor_depth, T)
    a_c, logpi_c, pcache = om.tanh_normal_sample(out_c, eps_cur, cfg)
    q_pi, caches_pi = om.critic_forward(pc, np.concatenate([a_c, obs], axis=1), cfg)
    terms = alpha * logpi_c.reshape(-1, 1) - q_pi.min(axis=0)
    wb = tw if tw is not None else np.ones((B, 1))
    g_logpi = (wb * alpha).reshape(-1) / B
    dq_pi = om.min_grad(q_pi) * (-wb / B)[None]
    g_a = np.zeros((B, A))
    for k in range(C):
        hs, t = caches_pi[k]
        _, dx = om.mh_backward(om.ens_slice(pc, k), hs, t, dq_pi[k], cfg.critic_depth, need_dx=True)
        g_a += dx[:, :A]
    dout = om.tanh_normal_backward(pcache, g_a, g_logpi, cfg)
    ga, _ = om.mh_backward(pa, hs_a, t_a, dout, cfg.actor_depth)
    if skip_task is not None:
        ga["head_W"][skip_task] = 0.0
        ga["head_b"][skip_task] = 0.0
    return float((wb * terms).mean()), untie_grad(om.flatten(ga, ash), actor_shapes(cfg), ash), logpi_c


# ------------------------------------------------------------------ the step
def update(cfg, state, batch, eps_next, eps_cur, skip_task=None):
    """``MTSAC._update_inner`` on the shared-head networks: critic, actor through the UPDATED critic, temperature.
    Returns (new_state, logs, internals); ``state`` is not mutated."""
    s = state.copy()
    batch = [np.asarray(b, np.float64) for b in batch]
    obs = batch[0]
    T, B = cfg.num_tasks, obs.shape[0]
    qf_loss, qf_values, gc = critic_loss_grad(cfg, s, batch, eps_next, skip_task)
    s.critic = om.adam_step(s.critic, om.clip_by_global_norm(gc, cfg.critic_max_grad_norm), s.critic_opt, cfg.critic_lr,
                            cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    s.critic_target = cfg.tau * s.critic + (1.0 - cfg.tau) * s.critic_target
    actor_loss, ga, logpi = actor_loss_grad(cfg, s, batch, eps_cur, skip_task)
    s.actor = om.adam_step(s.actor, om.clip_by_global_norm(ga, cfg.actor_max_grad_norm), s.actor_opt, cfg.actor_lr,
                           cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    task_ids = obs[:, -T:]
    lp = logpi.reshape(-1, 1) + cfg.target_entropy
    alpha_loss = (-(task_ids @ s.log_alpha.reshape(-1, 1)) * lp).mean()
    g_la = om.clip_by_global_norm((-(task_ids * lp)).sum(axis=0) / B, cfg.alpha_max_grad_norm)
    s.log_alpha = om.adam_step(s.log_alpha, g_la, s.alpha_opt, cfg.alpha_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    logs = {
        "losses/qf_values": qf_values,
        "losses/qf_loss": qf_loss,
        "metrics/critic_grad_magnitude": om.global_norm(gc),
        "metrics/critic_params_norm": om.global_norm(s.critic),
        "losses/actor_loss": actor_loss,
        "metrics/actor_grad_magnitude": om.global_norm(ga),
        "metrics/actor_params_norm": om.global_norm(s.actor),
        "metrics/explore_loss": 0.0,
        "losses/alpha_loss": float(alpha_loss),
        "alpha": float(np.exp(s.log_alpha).sum()),
    }
    return s, logs, dict(critic_grad=gc, actor_grad=ga)


# ------------------------------------------------------------------ per-task gradients
def task_grads(cfg, st, batch, eps_next, eps_cur):
    """(Gc [T][Pc], Ga [T][Pa]) of mtsac_task_gradients (oracle/conflict.py task_grads) in the Vanilla order."""
    Gc, Ga = oc.task_grads(cfg, tied_state(cfg, st), batch, eps_next, eps_cur)
    return (untie_rows(Gc, critic_shapes(cfg), om.critic_leaf_shapes(cfg)),
            untie_rows(Ga, actor_shapes(cfg), om.actor_leaf_shapes(cfg)))


def actor_task_grads(cfg, st, batch, eps_cur):
    """The training step's split actor loss with the explore term (tests/pcgrad_oracle.py _actor_task_grads):
    (G [T][Pa], loss_t, explore_t, logpi)."""
    G, loss_t, exp_t, logpi = po._actor_task_grads(cfg, tied_state(cfg, st), batch, eps_cur)
    return untie_rows(G, actor_shapes(cfg), om.actor_leaf_shapes(cfg)), loss_t, exp_t, logpi


def critic_losses(cfg, st, batch, eps_next):
    return po._critic_losses(cfg, tied_state(cfg, st), batch, eps_next)


def surgery_update(cfg, state, batch, eps_next, eps_cur, combine_critic, combine_actor):
    """One gradient-surgery step (the order of tests/pcgrad_oracle.py update): per-task critic gradients,
    ``combine_critic(Gc) -> g``, clip + Adam + Polyak; per-task actor gradients (explore term) through the
    UPDATED critic, ``combine_actor(Ga, task losses) -> g``, clip + Adam; temperature.
    Returns (new_state, logs, (Gc, Ga, critic task losses, actor task losses))."""
    s = state.copy()
    batch = [np.asarray(b, np.float64) for b in batch]
    obs = batch[0]
    T, B = cfg.num_tasks, obs.shape[0]
    qf_values, qf_loss = critic_losses(cfg, s, batch, eps_next)
    Gc, _ = task_grads(cfg, s, batch, eps_next, eps_cur)
    lc = critic_task_losses(cfg, s, batch, eps_next)
    gc = combine_critic(Gc, lc)
    s.critic = om.adam_step(s.critic, om.clip_by_global_norm(gc, cfg.critic_max_grad_norm), s.critic_opt, cfg.critic_lr,
                            cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    s.critic_target = cfg.tau * s.critic + (1.0 - cfg.tau) * s.critic_target
    Ga, loss_t, exp_t, logpi = actor_task_grads(cfg, s, batch, eps_cur)
    ga = combine_actor(Ga, loss_t)
    s.actor = om.adam_step(s.actor, om.clip_by_global_norm(ga, cfg.actor_max_grad_norm), s.actor_opt, cfg.actor_lr,
                           cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    task_ids = obs[:, -T:]
    lp = logpi.reshape(-1, 1) + cfg.target_entropy
    alpha_loss = (-(task_ids @ s.log_alpha.reshape(-1, 1)) * lp).mean()
    g_la = om.clip_by_global_norm((-(task_ids * lp)).sum(axis=0) / B, cfg.alpha_max_grad_norm)
    s.log_alpha = om.adam_step(s.log_alpha, g_la, s.alpha_opt, cfg.alpha_lr, cfg.adam_b1, cfg.adam_b2, cfg.adam_eps)
    logs = {
        "losses/qf_values": qf_values,
        "losses/qf_loss": qf_loss,
        "metrics/critic_grad_magnitude": om.global_norm(Gc.mean(axis=0)),
        "metrics/critic_params_norm": om.global_norm(s.critic),
        "losses/actor_loss": float(loss_t.mean()),
        "metrics/actor_grad_magnitude": om.global_norm(Ga.mean(axis=0)),
        "metrics/actor_params_norm": om.global_norm(s.actor),
        "metrics/explore_loss": float(exp_t.mean()),
        "losses/alpha_loss": float(alpha_loss),
        "alpha": float(np.exp(s.log_alpha).sum()),
    }
    return s, logs, (Gc, Ga, lc, loss_t)


def critic_task_losses(cfg, st, batch, eps_next):
    """Per-task critic loss values of the split pass: the MSE over the task's n rows and E members, with the
    "next" actions sampled from pi(.|s) of the OBSERVATIONS (as oracle/conflict.py task_grads does)."""
    obs, act, nobs, dones, rew = [np.asarray(b, np.float64) for b in batch]
    T, B = cfg.num_tasks, obs.shape[0]
    ts = tied_state(cfg, st)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc, pt = om.unflatten(ts.actor, ash), om.unflatten(ts.critic, csh), om.unflatten(ts.critic_target, csh)
    alpha = np.exp(obs[:, -T:] @ st.log_alpha.reshape(-1, 1))
    out, _, _ = om.mh_forward(pa, obs, cfg.actor_depth, T)
    a_n, lp_n, _ = om.tanh_normal_sample(out, eps_next, cfg)
    q_t, _ = om.critic_forward(pt, np.concatenate([a_n, nobs], axis=1), cfg)
    y = rew.reshape(B, 1) + (1.0 - dones.reshape(B, 1)) * cfg.gamma * (q_t.min(axis=0) - alpha * lp_n.reshape(-1, 1))
    q, _ = om.critic_forward(pc, np.concatenate([act, obs], axis=1), cfg)
    if cfg.clip:
        y, q = np.clip(y, -5000, 5000), np.clip(q, -5000, 5000)
    sq = ((q - y[None]) ** 2).mean(axis=0).reshape(-1)  # mean over members, per row
    tasks = np.argmax(obs[:, -T:], axis=1)
    return np.array([sq[tasks == t].mean() for t in range(T)])


# ------------------------------------------------------------------ rollout
def eval_action(cfg, st, obs):
    return om.eval_action(cfg, tied_state(cfg, st).actor, np.asarray(obs, np.float64))


def sample_action(cfg, st, obs, eps):
    return om.sample_action(cfg, tied_state(cfg, st).actor, np.asarray(obs, np.float64), np.asarray(eps, np.float64))
