"""Shapes, mid-training states and hyper-parameter sets shared by the SAC optimizer tests
(test_adam_ref_cpu.py on the CPU, test_gpu_optimizer.py on the GPU).  Everything here is numpy and the
float64 oracle; nothing touches the engine."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import adam_ref as ar
import grad_mag_ref as gm
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

# T, width, depth, rows per task (B = n T).  Which optimizer form each takes is asserted by
# test_gpu_optimizer.test_every_optimizer_form_occurs.
CASES = {
    "tiny": dict(T=3, W=16, depth=3, n=4),        # one partial tile per leaf
    "deep2_w40": dict(T=2, W=40, depth=2, n=4),   # padded leading dimension (64) != width
    "w100_d2": dict(T=3, W=100, depth=2, n=5),    # 2 x 2 tiles with ragged edges
    # actor input 64 = exactly one tile row, critic input 68 = one row past it, width 64 + 8
    "rows64": dict(T=25, W=72, depth=3, n=2),
    "w64_d1": dict(T=2, W=64, depth=1, n=8),      # no hidden kernel: plane segments under split precisions
    "mt50_w400": dict(T=50, W=400, depth=3, n=2),  # 7 x 7 ragged tiles, E = 2 Polyak tiles
}
SMALL = ("tiny", "w100_d2", "w64_d1")  # crossed with the hyper-parameter sets and the clips
PRECISIONS = {"fp32": 0, "split3": 1, "bf16": 2, "split2h": 3}
COUNTS_B = (1, 9, 99999)  # actor, critic, alpha


def oracle_config(name: str, T: int | None = None, **over) -> om.OracleConfig:
    c = CASES[name] if name in CASES else dict(T=T, W=16, depth=2, n=2)  # part 2: the temperature shapes
    T = c["T"]
    kw = dict(num_tasks=T, obs_dim=39 + T, actor_width=c["W"], critic_width=c["W"], actor_depth=c["depth"],
              critic_depth=c["depth"], actor_max_grad_norm=None, critic_max_grad_norm=None,
              alpha_max_grad_norm=None)
    kw.update(over)
    return om.OracleConfig(**kw)


def rows_per_task(name: str) -> int:
    return CASES[name]["n"] if name in CASES else 2


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def base_state(name: str, T: int | None = None, seed: int = 11):
    """(state, batch, eps_next, eps_cur, batch2, eps_next2, eps_cur2): float32 values held in float64.
    om.initialize parameters, hidden biases N(0, 0.01), target = critic + N(0, 1e-3), log_alpha
    U(-0.3, 0.3), zero moments; a second batch and noise for the tests that run two steps."""
    cfg = oracle_config(name, T)
    T = cfg.num_tasks
    st = om.initialize(cfg, seed=seed, dtype=np.float64)
    rng = np.random.default_rng(seed + 1)
    for attr, shapes in (("actor", om.actor_leaf_shapes(cfg)), ("critic", om.critic_leaf_shapes(cfg))):
        p = om.unflatten(getattr(st, attr), shapes)
        for k in p:
            if k.startswith("b"):
                p[k] = rng.normal(0.0, 0.01, p[k].shape)
        setattr(st, attr, _r32(om.flatten(p, shapes)))
    st.critic_target = _r32(st.critic + rng.normal(0.0, 1e-3, st.critic.shape))
    st.log_alpha = _r32(rng.uniform(-0.3, 0.3, T))
    B = rows_per_task(name) * T
    out = [st]
    for s in (0, 1):
        batch = synthetic_batch(T, B, seed=100 + s, dtype=np.float32)
        en, ec = synthetic_eps(B, seed=200 + s, dtype=np.float32)
        out += [batch, en, ec]
    return tuple(out)


ENGINE_TASKS = 64  # mtsac_create: at most 64 tasks per engine


def owned_tasks(T: int) -> int:
    """More than 64 tasks exist only as task shards: the engine of such a case owns tasks [0, 64) of T.
    Its log_alpha, temperature moments and one-hot columns are global (T), its heads and rows local."""
    return min(T, ENGINE_TASKS)


def local_flat(cfg: om.OracleConfig, flat, net: str):
    """A flat actor / critic vector of the oracle with the head leaves cut to the owned tasks."""
    tc = owned_tasks(cfg.num_tasks)
    if net == "alpha" or tc == cfg.num_tasks:
        return flat
    shapes = om.critic_leaf_shapes(cfg) if net == "critic" else om.actor_leaf_shapes(cfg)
    p = om.unflatten(np.asarray(flat), shapes)
    out = []
    for k, _ in shapes:
        v = p[k]
        if k.startswith("head"):
            v = v[:, :tc] if net == "critic" else v[:tc]
        out.append(v.reshape(-1))
    return np.concatenate(out)


def local_rows(cfg: om.OracleConfig, batch, eps_next, eps_cur):
    """The rows of the owned tasks, in the order they have (row = i T + t becomes i tc + t)."""
    T, tc = cfg.num_tasks, owned_tasks(cfg.num_tasks)
    if tc == T:
        return batch, eps_next, eps_cur
    keep = np.argmax(batch[0][:, -T:], axis=1) < tc
    return tuple(b[keep] for b in batch), eps_next[keep], eps_cur[keep]


def f64(batch):
    return [np.asarray(b, np.float64) for b in batch]


@functools.lru_cache(maxsize=None)
def oracle_pass(name: str, T: int | None = None, clip_tw: bool = False):
    """The oracle's plain step from the base state (zero moments, no clips, default hyper-parameters):
    dict with the new state, logs, internals (critic_grad, actor_grad, alpha_grad, logpi_cur, ...) and
    the gradient magnitudes of grad_mag_ref."""
    cfg = oracle_config(name, T, clip=clip_tw, use_task_weights=clip_tw)
    st, batch, en, ec = base_state(name, T)[:4]
    new, logs, internals, mags = gm.update_with_magnitudes(cfg, st, f64(batch), en.astype(np.float64),
                                                           ec.astype(np.float64))
    return dict(cfg=cfg, new=new, logs=logs, mag_critic=mags["critic"][0], mag_actor=mags["actor"][0],
                plain_critic=mags["critic"][1], plain_actor=mags["actor"][1], **internals)


@dataclasses.dataclass
class HyperSet:
    """One run's optimizer settings: per-network learning rates, the shared Adam constants, the Adam
    counts before the step (actor, critic, alpha)."""
    actor_lr: float = 3e-4
    critic_lr: float = 3e-4
    alpha_lr: float = 3e-4
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-5
    tau: float = 0.005
    counts: tuple = (0, 0, 0)

    def hyper(self, net: str) -> ar.Hyper:
        return ar.Hyper(getattr(self, net + "_lr"), self.b1, self.b2, self.eps, self.tau)


def start_moments(name: str, hs: HyperSet, T: int | None = None):
    """{net: (mu0, nu0)} float32.  Count 0 is reachable with zero moments only; every other count gets
    the generator's moments over the oracle's gradient of the case."""
    o = oracle_pass(name, T)
    out = {}
    for i, net in enumerate(("actor", "critic", "alpha")):
        g = local_flat(o["cfg"], o[net + "_grad"], net)
        if hs.counts[i] == 0:
            out[net] = (np.zeros(g.size, np.float32), np.zeros(g.size, np.float32))
        else:
            out[net] = ar.reachable_moments(g, hs.hyper(net), seed=31 + i)
    return out


def median_sqrt_nu_hat(name: str, hs: HyperSet) -> float:
    """Median over the actor's and critic's elements with a gradient of sqrt(nu_hat) after the step, from
    the oracle's gradient (the engine's differs from it by rounding only)."""
    o = oracle_pass(name)
    mom = start_moments(name, hs)
    vals = []
    for i, net in enumerate(("actor", "critic")):
        g = o[net + "_grad"]
        nu = (1 - ar.f32(hs.b2)) * g * g + ar.f32(hs.b2) * mom[net][1].astype(np.float64)
        vals.append(np.sqrt(nu[nu > 0] / (1 - ar.f32(hs.b2) ** (hs.counts[i] + 1))))
    return float(np.median(np.concatenate(vals)))


@functools.lru_cache(maxsize=None)
def hyper_set(name: str, which: str) -> HyperSet:
    """(a) defaults from count 0; (b) defaults from counts (1, 9, 99999); (c) every constant off its
    default, per-network learning rates, and adam_eps at the case's median sqrt(nu_hat), so that eps
    changes the step by tens of percent instead of 1e-5 / |g|."""
    if which == "a":
        return HyperSet()
    if which == "b":
        return HyperSet(counts=COUNTS_B)
    assert which == "c"
    hs = HyperSet(actor_lr=1e-3, critic_lr=2e-4, alpha_lr=5e-4, b1=0.8, b2=0.99, tau=0.05, counts=COUNTS_B)
    med = median_sqrt_nu_hat(name, hs)
    hs.eps = ar.f32(med)
    assert med / 10 <= hs.eps <= med * 10
    return hs


def clip_thresholds(name: str, which: str, T: int | None = None):
    """(actor, critic, alpha) max_grad_norm: none, 'quarter' = 0.25 ||g|| (clipped), 'four' = 4 ||g|| (kept),
    'zero' = 0.0 for actor and critic (the gradient is clipped away; the old momentum still moves the
    parameters).  ||g|| is the oracle's; the engine's differs from it in the seventh digit."""
    if which == "none":
        return (None, None, None)
    o = oracle_pass(name, T)
    n = [float(np.linalg.norm(o[k])) for k in ("actor_grad", "critic_grad", "alpha_grad")]
    if which == "zero":
        return (0.0, 0.0, None)
    f = {"quarter": 0.25, "four": 4.0}[which]
    return tuple(ar.f32(f * x) for x in n)
