"""GPU parity of the full MTSAC gradient step against the oracle.

The engine (libmtsac.so, fp32 MFMA) and the float64 numpy oracle start from the
same fp32 parameters and see the same batch and the same injected noise.  Bar
(BASELINE.json north_star): fp32 losses within 1e-5 relative; the other logs,
parameters and optimizer state within the fp32-vs-fp64 tolerances written below.
"""

from __future__ import annotations

import numpy as np
import pytest

from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5


def _engine_for(cfg: om.OracleConfig, capacity=256, graph=False, precision=0):
    from mtrl_amd.engine import MTSACEngine, make_config

    c = make_config(
        precision=precision,
        num_tasks=cfg.num_tasks, task_count=cfg.num_tasks, obs_dim=cfg.obs_dim, action_dim=cfg.action_dim,
        actor_width=cfg.actor_width, actor_depth=cfg.actor_depth, critic_width=cfg.critic_width,
        critic_depth=cfg.critic_depth, num_critics=cfg.num_critics, batch_per_task=BATCH_PER_TASK[0],
        capacity=capacity, gamma=cfg.gamma, tau=cfg.tau, clip=int(cfg.clip), use_task_weights=int(cfg.use_task_weights),
        actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm,
    )
    e = MTSACEngine(c)
    e.enable_graph(graph)
    return e


BATCH_PER_TASK = [4]


def _load_state(eng, st: om.MTSACState):
    from mtrl_amd import _lib as L

    eng.set_params(L.ACTOR, st.actor)
    eng.set_params(L.CRITIC, st.critic)
    eng.set_params(L.CRITIC_TARGET, st.critic_target)
    eng.set_params(L.LOG_ALPHA, st.log_alpha)


def _f32_state(cfg, seed):
    st = om.initialize(cfg, seed=seed, dtype=np.float64)
    for name in ("actor", "critic", "critic_target", "log_alpha"):
        setattr(st, name, getattr(st, name).astype(np.float32).astype(np.float64))
    return st


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


CONFIGS = {
    "tiny": dict(num_tasks=3, width=16, n=4),
    "mt10_w64": dict(num_tasks=10, width=64, n=8),
    "clip_tw": dict(num_tasks=3, width=32, n=4, clip=True, use_task_weights=True),
    "deep2": dict(num_tasks=2, width=40, n=4, depth=2),
    "mt10_w400": dict(num_tasks=10, width=400, n=128),  # S1 / C1 at full batch
    "mt50_w400": dict(num_tasks=50, width=400, n=16),
    # headline widths (S2 with its clip=True, S3's 50 tasks) at a batch the float64 oracle runs in seconds
    "mt10_w2048_clip": dict(num_tasks=10, width=2048, n=16, clip=True),
    "mt50_w2048": dict(num_tasks=50, width=2048, n=4),
    # the other action and ensemble sizes mtsac_create accepts: the padded critic input widths, the W0 action
    # rows and the target entropy around the head kernels (tests/test_gpu_head_kernels.py has the kernels alone)
    "a1_c1": dict(num_tasks=3, width=16, n=4, action_dim=1, num_critics=1),
    "a3_c3": dict(num_tasks=3, width=16, n=4, action_dim=3, num_critics=3),
    "a2_c4": dict(num_tasks=3, width=16, n=4, action_dim=2, num_critics=4),
}


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_update_matches_oracle(name, precision):
    from mtrl_amd import _lib as L

    spec = CONFIGS[name]
    T, W, n = spec["num_tasks"], spec["width"], spec["n"]
    A = spec.get("action_dim", 4)
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A,
                          num_critics=spec.get("num_critics", 2),
                          actor_depth=spec.get("depth", 3), critic_depth=spec.get("depth", 3),
                          clip=spec.get("clip", False), use_task_weights=spec.get("use_task_weights", False))
    BATCH_PER_TASK[0] = n
    B = n * T
    st = _f32_state(cfg, seed=11)
    eng = _engine_for(cfg, precision=precision)
    _load_state(eng, st)
    for step in range(3):
        batch = synthetic_batch(T, B, action_dim=A, seed=100 + step, dtype=np.float32)
        en, ec = synthetic_eps(B, action_dim=A, seed=200 + step, dtype=np.float32)
        st, want = om.update(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64),
                             ec.astype(np.float64))
        eng.update(batch, en, ec)
        got = eng.logs()
        for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values"):
            if k == "losses/alpha_loss" and step == 0:
                assert abs(got[k]) < 1e-6  # log_alpha = 0 at init -> loss is exactly 0
                continue
            tol = LOSS_RTOL
            scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
            assert abs(got[k] - want[k]) <= tol * scale, (name, step, k, got[k], want[k])
        for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
                  "metrics/actor_params_norm", "alpha"):
            assert _rel(got[k], want[k]) < 1e-4, (name, step, k, got[k], want[k])
        assert got["metrics/explore_loss"] == 0.0
    # parameters / optimizer state after 3 steps: elementwise fp32 tolerance
    for which, ref in ((L.ACTOR, st.actor), (L.CRITIC, st.critic), (L.CRITIC_TARGET, st.critic_target),
                       (L.LOG_ALPHA, st.log_alpha)):
        g = eng.get_params(which).astype(np.float64)
        d = np.abs(g - ref)
        # Adam moves every coordinate by ~lr; a coordinate whose gradient is ~0 may get its sign flipped by
        # fp32 rounding, so bound the typical error tightly and the worst case by 2 * lr * steps.
        assert np.median(d) < 1e-6, (which, np.median(d))
        assert d.max() < 2 * 3e-4 * 3 + 1e-6, (which, d.max())
    assert eng.get_adam_count(0) == 3 and eng.get_adam_count(1) == 3 and eng.get_adam_count(2) == 3
    eng.close()


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
def test_graph_replay_is_deterministic_and_matches_eager(precision):
    from mtrl_amd import _lib as L

    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    BATCH_PER_TASK[0] = n
    st = _f32_state(cfg, seed=3)
    outs = []
    for graph in (False, True, True):
        eng = _engine_for(cfg, capacity=64, graph=graph, precision=precision)
        _load_state(eng, st)
        eng.buffer_fill_synthetic(99)
        eng.seed_rng(1)
        eng.update_many(4)
        outs.append((eng.logs(), eng.get_params(L.ACTOR), eng.get_params(L.CRITIC), eng.get_rng_state()))
        eng.close()
    for o in outs[1:]:
        assert o[0] == outs[0][0]
        np.testing.assert_array_equal(o[1], outs[0][1])
        np.testing.assert_array_equal(o[2], outs[0][2])
        assert o[3] == outs[0][3]


def test_device_sampled_update_matches_oracle_with_same_indices():
    """The device index stream + gather feed the update exactly like buffer.sample()."""
    from oracle.buffer import MultiTaskReplayBufferOracle

    T, W, n, cap = 3, 16, 4, 32
    D, A = 39 + T, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=D, actor_width=W, critic_width=W)
    BATCH_PER_TASK[0] = n
    st = _f32_state(cfg, seed=5)
    eng = _engine_for(cfg, capacity=cap)
    _load_state(eng, st)
    orc = MultiTaskReplayBufferOracle(cap * T, T, D, A, seed=1)
    eng.seed_rng(1)
    rng = np.random.default_rng(0)
    for s in range(20):
        o = np.zeros((T, D), np.float32); o[:, :39] = rng.standard_normal((T, 39)); o[np.arange(T), 39 + np.arange(T)] = 1
        no = o.copy(); no[:, :39] = rng.standard_normal((T, 39))
        a = rng.uniform(-1, 1, (T, A)).astype(np.float32)
        r = rng.uniform(0, 10, T).astype(np.float32)
        d = (rng.uniform(size=T) < 0.2).astype(np.float32)
        eng.buffer_add(o, no, a, r, d)
        orc.add(o, no, a, r, d)
    # the oracle takes its noise as an argument (the device stream itself is held to its host model in
    # test_gpu_noise_stream.py), so draw the batch on both sides and inject eps via a user batch
    idx, batch = eng.sample()
    want_idx = orc.sample_indices(n * T)
    np.testing.assert_array_equal(idx, want_idx)
    en, ec = synthetic_eps(n * T, seed=9, dtype=np.float32)
    st2, want = om.update(cfg, st, [b.astype(np.float64) for b in orc.gather(want_idx)], en.astype(np.float64),
                          ec.astype(np.float64))
    eng.update(batch, en, ec)
    got = eng.logs()
    for k in ("losses/qf_loss", "losses/actor_loss"):
        assert abs(got[k] - want[k]) <= LOSS_RTOL * abs(want[k]), (k, got[k], want[k])
    eng.close()


def test_rollout_actions_match_oracle():
    from mtrl_amd import _lib as L

    T, W = 10, 64
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    BATCH_PER_TASK[0] = 2
    st = _f32_state(cfg, seed=8)
    eng = _engine_for(cfg, capacity=16)
    _load_state(eng, st)
    obs = synthetic_batch(T, T, seed=3, dtype=np.float32)[0]
    eps = np.random.default_rng(4).standard_normal((T, 4)).astype(np.float32)
    np.testing.assert_allclose(eng.eval_action(obs), om.eval_action(cfg, st.actor, obs.astype(np.float64)),
                               rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(eng.sample_action(obs, eps),
                               om.sample_action(cfg, st.actor, obs.astype(np.float64), eps.astype(np.float64)),
                               rtol=1e-5, atol=1e-6)
    eng.close()


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_rccl_single_rank_graph_path(graph, precision):
    """The RCCL all-reduce points (per-layer buckets on their own stream, then layer 0 and the
    scalar tail), captured in the hipGraph or issued eagerly (1-rank communicator): same
    results as the communicator-free engine."""
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine

    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    BATCH_PER_TASK[0] = n
    st = _f32_state(cfg, seed=4)
    outs = []
    for use_comm in (False, True):
        eng = _engine_for(cfg, capacity=64, graph=graph, precision=precision)
        _load_state(eng, st)
        if use_comm:
            eng.comm_init(MTSACEngine.comm_unique_id(), 1, 0)
        eng.buffer_fill_synthetic(5)
        eng.seed_rng(2)
        eng.update_many(3)
        outs.append((eng.logs(), eng.get_params(L.ACTOR)))
        eng.close()
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
