"""The whole MTSAC step with wide action spaces (action_dim 5 .. 64, the wide head kernels of
mtrl_amd/csrc/heads_wide.h) against the float64 oracle, in the form and at the bars of
tests/test_gpu_update.py: losses within 1e-5 relative, norms and alpha within 1e-4, parameters' median error below
1e-6 and maximum below 2 lr steps + 1e-6, Adam counts.  Then every path around the step that sizes something
from A: graph replay, rollout actions, the synthetic buffer fill, the in-process shard, one PCGrad step, the
conflict metrics and the compat trainer end to end."""

from __future__ import annotations

import functools
import threading
from dataclasses import dataclass

import numpy as np
import pytest

import test_gpu_update as TU
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL = TU.LOSS_RTOL

CONFIGS = {
    "a5": dict(num_tasks=3, width=16, n=4, action_dim=5),
    "a5_c1": dict(num_tasks=3, width=16, n=4, action_dim=5, num_critics=1),
    "a8": dict(num_tasks=3, width=16, n=4, action_dim=8),
    "a19": dict(num_tasks=3, width=16, n=4, action_dim=19),
    "a64": dict(num_tasks=3, width=16, n=4, action_dim=64),
    "t9_w512_a19": dict(num_tasks=9, width=512, n=16, action_dim=19),  # the HumanoidBench shape: Box(19), nine tasks
    "clip_tw_a6": dict(num_tasks=3, width=32, n=4, action_dim=6, clip=True, use_task_weights=True),
}


def _cfg(spec):
    T, W = spec["num_tasks"], spec["width"]
    return om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=spec["action_dim"],
                           num_critics=spec.get("num_critics", 2), clip=spec.get("clip", False),
                           use_task_weights=spec.get("use_task_weights", False))


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """Three oracle steps from seed 11 on the batches 100 + step and noise 200 + step: computed once per shape and
    shared by the precisions (never mutated)."""
    spec = CONFIGS[name]
    T, n, A = spec["num_tasks"], spec["n"], spec["action_dim"]
    cfg = _cfg(spec)
    st0 = TU._f32_state(cfg, seed=11)
    st, steps = st0, []
    for step in range(3):
        batch = synthetic_batch(T, n * T, action_dim=A, seed=100 + step, dtype=np.float32)
        en, ec = synthetic_eps(n * T, action_dim=A, seed=200 + step, dtype=np.float32)
        st, want = om.update(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64), ec.astype(np.float64))
        steps.append((batch, en, ec, want))
    return cfg, st0, st, steps


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_update_matches_oracle(name, precision):
    from mtrl_amd import _lib as L

    cfg, st0, st, steps = _oracle_run(name)
    TU.BATCH_PER_TASK[0] = CONFIGS[name]["n"]
    eng = TU._engine_for(cfg, precision=precision)
    TU._load_state(eng, st0)
    for step, (batch, en, ec, want) in enumerate(steps):
        eng.update(batch, en, ec)
        got = eng.logs()
        print(name, precision, step, {k: (got[k], want[k]) for k in got if k in want})
        for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values"):
            if k == "losses/alpha_loss" and step == 0:
                assert abs(got[k]) < 1e-6  # log_alpha = 0 at init -> loss is exactly 0
                continue
            scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
            assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (name, step, k, got[k], want[k])
        for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
                  "metrics/actor_params_norm", "alpha"):
            assert TU._rel(got[k], want[k]) < 1e-4, (name, step, k, got[k], want[k])
        assert got["metrics/explore_loss"] == 0.0
    for which, ref in ((L.ACTOR, st.actor), (L.CRITIC, st.critic), (L.CRITIC_TARGET, st.critic_target),
                       (L.LOG_ALPHA, st.log_alpha)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (which, np.median(d))
        assert d.max() < 2 * 3e-4 * 3 + 1e-6, (which, d.max())
    assert eng.get_adam_count(0) == 3 and eng.get_adam_count(1) == 3 and eng.get_adam_count(2) == 3
    eng.close()


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
def test_wide_graph_replay_matches_eager(precision):
    from mtrl_amd import _lib as L

    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=19)
    TU.BATCH_PER_TASK[0] = n
    st = TU._f32_state(cfg, seed=3)
    outs = []
    for graph in (False, True, True):
        eng = TU._engine_for(cfg, capacity=64, graph=graph, precision=precision)
        TU._load_state(eng, st)
        eng.buffer_fill_synthetic(99)
        eng.seed_rng(1)
        eng.update_many(4)
        outs.append((eng.logs(), eng.get_params(L.ACTOR), eng.get_params(L.CRITIC), eng.get_rng_state()))
        eng.close()
    assert all(np.isfinite(v) for v in outs[0][0].values())
    for o in outs[1:]:
        assert o[0] == outs[0][0]
        np.testing.assert_array_equal(o[1], outs[0][1])
        np.testing.assert_array_equal(o[2], outs[0][2])
        assert o[3] == outs[0][3]


def test_wide_rollout_actions_match_oracle():
    T, W, A = 10, 64, 19
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A)
    TU.BATCH_PER_TASK[0] = 2
    st = TU._f32_state(cfg, seed=8)
    eng = TU._engine_for(cfg, capacity=16)
    TU._load_state(eng, st)
    obs = synthetic_batch(T, T, action_dim=A, seed=3, dtype=np.float32)[0]
    eps = np.random.default_rng(4).standard_normal((T, A)).astype(np.float32)
    np.testing.assert_allclose(eng.eval_action(obs), om.eval_action(cfg, st.actor, obs.astype(np.float64)),
                               rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(eng.sample_action(obs, eps),
                               om.sample_action(cfg, st.actor, obs.astype(np.float64), eps.astype(np.float64)),
                               rtol=1e-5, atol=1e-6)
    eng.close()


def test_wide_buffer_fill_covers_every_action_column():
    T, W, n, cap = 3, 16, 4, 32
    TU.BATCH_PER_TASK[0] = n
    acts = {}
    for A in (4, 6):
        cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A)
        eng = TU._engine_for(cfg, capacity=cap)
        eng.buffer_fill_synthetic(7)
        acts[A] = eng.buffer_read(0, cap)[2]
        if A == 6:
            eng.seed_rng(1)
            eng.update_many(2)
            assert all(np.isfinite(v) for v in eng.logs().values())
        eng.close()
    assert acts[6].shape == (cap, T, 6)
    assert np.isfinite(acts[6]).all() and (np.abs(acts[6]) <= 1).all()
    assert (np.abs(acts[6][..., 4:]) > 0).all(), "action columns past the fourth were left unfilled"
    np.testing.assert_array_equal(acts[6][..., :4], acts[4])  # columns 0 .. 3 are the draw they always were


def test_wide_sharded_update_matches_single():
    """Two in-process shards of a T = 5, A = 6 problem against the single engine (tests/test_gpu_shard.py's bars)."""
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config
    from mtrl_amd.init import init_mtsac
    from mtrl_amd.shard import InProcessAllReduce, local_rows, shard_tasks

    T, W, n, world, A = 5, 32, 4, 2, 6
    D, B = 39 + T, n * T

    def mk(begin, count):
        e = MTSACEngine(make_config(num_tasks=T, task_begin=begin, task_count=count, obs_dim=D, action_dim=A,
                                    actor_width=W, critic_width=W, batch_per_task=n, capacity=16))
        a, c = init_mtsac(T, D, A, W, 3, W, 3, 2, seed=3, task_begin=begin, task_count=count)
        e.set_params(L.ACTOR, a)
        e.set_params(L.CRITIC, c)
        e.set_params(L.CRITIC_TARGET, c)
        return e

    single = mk(0, T)
    shards = [mk(*shard_tasks(T, world, r)) for r in range(world)]
    group = InProcessAllReduce(world)
    for r, e in enumerate(shards):
        e.set_allreduce_hook(group.hook(r))
    for step in range(2):
        batch = synthetic_batch(T, B, action_dim=A, seed=50 + step, dtype=np.float32)
        en, ec = synthetic_eps(B, action_dim=A, seed=60 + step, dtype=np.float32)
        single.update(batch, en, ec)
        want1 = single.logs()
        errs = []

        def run(r):
            try:
                rows = local_rows(T, n, *shard_tasks(T, world, r))
                shards[r].update(tuple(x[rows] for x in batch), en[rows], ec[rows])
            except Exception as ex:  # pragma: no cover
                errs.append(ex)

        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs
        logs = [e.logs() for e in shards]
        assert all(lg == logs[0] for lg in logs)
        for k in ("losses/qf_loss", "losses/actor_loss", "losses/qf_values"):
            assert abs(logs[0][k] - want1[k]) <= 1e-5 * max(abs(want1[k]), 1e-3), (step, k, logs[0][k], want1[k])
        for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
                  "metrics/actor_params_norm", "alpha", "losses/alpha_loss"):
            assert abs(logs[0][k] - want1[k]) <= 1e-4 * max(abs(want1[k]), 1e-3), (step, k, logs[0][k], want1[k])
    for e in shards + [single]:
        e.close()


# T, W, n, A, seed.  The seed was picked on the CPU from the oracle alone (as tests/test_gpu_pcgrad.py's): at 32 the
# smallest |cos| of a projection decision is 7.7e-3 and both networks project (seed 23 gives 8e-4)
PCGRAD_CASE = (3, 32, 4, 6, 32)


def test_wide_pcgrad_step_matches_oracle():
    import pcgrad_oracle as po
    import test_gpu_pcgrad as TP
    from mtrl_amd import _lib as L

    T, W, n, A, seed = PCGRAD_CASE
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A)
    st0 = po.head_init_state(cfg, seed, head_bound=1.0)
    rng = np.random.default_rng(seed + 7)
    batch = synthetic_batch(T, n * T, action_dim=A, seed=seed + 100, dtype=np.float32)
    en = np.repeat(rng.standard_normal((n, A)), T, axis=0).astype(np.float32)
    ec = np.repeat(rng.standard_normal((n, A)), T, axis=0).astype(np.float32)
    pc, pa = rng.permutation(T), rng.permutation(T)
    st, want, margins = po.update(cfg, st0.copy(), batch, en.astype(np.float64), ec.astype(np.float64), pc, pa)
    assert min(margins) >= 1e-3, margins  # the decisions must not hinge on rounding
    eng = TP._engine(T, W, n, 1, capacity=64, action_dim=A, actor_max_grad_norm=cfg.actor_max_grad_norm,
                     critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_pcgrad(True)
    TP._load_state(eng, st0)
    eng.pcgrad_set_order(pc, pa)
    eng.update(batch, en, ec)
    got, got_pc = eng.logs(), eng.pcgrad_logs()
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/qf_values", "metrics/explore_loss"):
        scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
        assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (k, got[k], want[k])
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
              "metrics/actor_params_norm", "alpha"):
        assert abs(got[k] - want[k]) < 1e-4 * abs(want[k]), (k, got[k], want[k])
    for net in ("critic", "actor"):
        assert got_pc[f"metrics/{net}_n_grad_conflicts"] == want[f"metrics/{net}_n_grad_conflicts"]
    for which, ref in ((L.ACTOR, st.actor), (L.CRITIC, st.critic)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6 and d.max() < 2 * 3e-4 + 1e-6, (which, np.median(d), d.max())
    eng.close()


def test_wide_compute_weights_matches_oracle_metrics():
    from mtrl_amd import _lib as L
    from mtrl_amd import conflict as mc
    from mtrl_amd.engine import MTSACEngine, make_config
    from oracle import conflict as oc

    T, W, n, A, seed = 6, 64, 8, 6, 21
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A)
    st = om.initialize(cfg, seed=seed)
    st.log_alpha = np.random.default_rng(seed).uniform(-0.3, 0.3, T)
    for k in ("actor", "critic", "critic_target", "log_alpha"):
        setattr(st, k, getattr(st, k).astype(np.float32).astype(np.float64))
    e = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, action_dim=A, actor_width=W, critic_width=W,
                                batch_per_task=n, capacity=64, precision=1))
    TU._load_state(e, st)
    batch = synthetic_batch(T, n * T, action_dim=A, seed=seed + 2, dtype=np.float32)
    en, ec = synthetic_eps(n * T, action_dim=A, seed=seed + 3, dtype=np.float32)
    logs = mc.compute_weights(e, batch, en, ec)
    Gc, Ga = oc.task_grads(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64), ec.astype(np.float64))
    for net, which, Gw in (("critic", 0, Gc), ("actor", 1, Ga)):
        G = e.get_task_gradients(which).astype(np.float64)
        for t in range(T):  # tests/test_gpu_conflict.py: per-task gradients within 1e-5 of the task's largest entry
            assert np.abs(G[t] - Gw[t]).max() <= 1e-5 * np.abs(Gw[t]).max(), (net, t)
        for k, v in oc.network_metrics(G).items():
            g = np.asarray(logs[f"{net}_{k}"], np.float64)
            assert g.shape == np.shape(v), (net, k)
            np.testing.assert_allclose(g, v, rtol=2e-5, atol=1e-6, err_msg=f"{net}_{k}")
    assert len(logs) == 66
    e.close()


# ------------------------------------------------------------------ the compat trainer on Box(19), nine tasks
class _WideVecEnv:
    """tests/fake_env.py's vector env with a 19-dimensional action space (that one is fixed at 4)."""

    def __init__(self, T, A, max_steps=7, seed=0):
        from mtrl_amd.compat.envs.spaces import Box

        self.num_envs = self.T = T
        self.A, self.max_steps = A, max_steps
        self.rng = np.random.default_rng(seed)
        self.action_space = Box(-1.0, 1.0, shape=(T, A), dtype=np.float32, seed=seed)
        self.t, self.ret = np.zeros(T, int), np.zeros(T)

    def _obs(self):
        o = np.zeros((self.T, 39 + self.T), np.float64)
        o[:, :39] = self.rng.standard_normal((self.T, 39))
        o[np.arange(self.T), 39 + np.arange(self.T)] = 1.0
        return o

    def reset(self, seed=None):
        self.t[:] = 0
        self.ret[:] = 0
        return self._obs(), {}

    def step(self, actions):
        actions = np.asarray(actions)
        assert actions.shape == (self.T, self.A) and np.all(np.abs(actions) <= 1)
        self.t += 1
        r = 1.0 - np.abs(actions).mean(axis=1)
        self.ret += r
        obs = self._obs()
        trunc = self.t >= self.max_steps
        infos = {}
        if trunc.any():
            infos["final_obs"] = np.array([obs[i].copy() if trunc[i] else None for i in range(self.T)], dtype=object)
            infos["final_info"] = {"episode": {"r": self.ret.copy(), "l": self.t.copy()}}
            self.t[trunc] = 0
            self.ret[trunc] = 0
        return obs, r, np.zeros(self.T, bool), trunc, infos


def _wide_env_config(T, A):
    from mtrl_amd.compat.envs import MetaworldConfig
    from mtrl_amd.compat.envs.spaces import Box

    @dataclass(frozen=True)
    class WideConfig(MetaworldConfig):
        @property
        def num_tasks(self):
            return T

        @property
        def action_space(self):
            return Box(np.full(A, -1.0, np.float32), np.full(A, 1.0, np.float32), dtype=np.float32)

        @property
        def observation_space(self):
            return Box(np.full(39 + T, -np.inf), np.full(39 + T, np.inf), dtype=np.float64)

    return WideConfig(env_id="wide")


def test_wide_compat_trainer_end_to_end():
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.rl.algorithms import MTSAC, MTSACConfig

    T, A = 9, 19
    env_config = _wide_env_config(T, A)
    net = lambda: MultiHeadConfig(num_tasks=T, width=64, optimizer=OptimizerConfig(max_grad_norm=1.0))
    alg = MTSACConfig(num_tasks=T, gamma=0.99, actor_config=ContinuousActionPolicyConfig(network_config=net()),
                      critic_config=QValueFunctionConfig(network_config=net()), num_critics=2)
    train = OffPolicyTrainingConfig(total_steps=T * 40, buffer_size=50 * T, batch_size=8 * T, warmstart_steps=20,
                                    evaluation_frequency=0)
    agent = MTSAC.initialize(alg, env_config, seed=1)
    assert agent.engine.action_dim == A
    agent = agent.train(train, _WideVecEnv(T, A), None, env_config)
    assert agent.engine.get_adam_count(0) == 40 - 21  # one update per step once global_step > warmstart
    assert all(np.isfinite(v) for v in agent.engine.logs().values())
    act = agent.eval_action(_WideVecEnv(T, A).reset()[0])
    assert act.shape == (T, A) and np.all(np.abs(act) <= 1)
    state = agent.state_dict()
    a2 = MTSAC.initialize(alg, env_config, seed=7)
    a2.load_state_dict(state)
    for w in range(10):
        np.testing.assert_array_equal(agent.engine.get_params(w), a2.engine.get_params(w))
    assert [agent.engine.get_adam_count(i) for i in range(3)] == [a2.engine.get_adam_count(i) for i in range(3)]
