"""CAGrad on the GPU (mtrl/optim/cagrad.py, CAGradConfig on both optimizers).

* the solve kernel alone (cagrad.hip) on a matrix loaded with set_task_gradients, against
  mtrl_amd.cagrad.cagrad_from_gram on the device Gram, from the reference's start and from w0 = 1 (where
  the search is not trivial), then the combine with the returned weights;
* three CAGrad steps against the float64 oracle (tests/cagrad_oracle.py) with injected noise, at fp32,
  split3 and split2h, and one step at T = 50: nothing in the step hinges on a rounding-sensitive decision
  (the reference's search never leaves its start), so everything is compared;
* the device path (update_many), the mode's contracts, and the compat trainer with CAGradConfig on both
  networks.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import cagrad_oracle as co
import pcgrad_oracle as po
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5  # tests/test_gpu_pcgrad.py
NORM_RTOL = 1e-4
# obj_hist: 10x the bound of test_cagrad_cpu.py::test_gram_form_matches_literal_statement (its floor, 1e-12,
# decided every case there), relative to the largest entry
HIST_RTOL = 1e-11


def _engine(T, W, n, precision=1, capacity=64, **kw):
    from mtrl_amd.engine import MTSACEngine, make_config

    return MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W,
                                   batch_per_task=n, capacity=max(n, capacity), precision=precision, **kw))


def _load_state(eng, st):
    from mtrl_amd import _lib as L

    eng.set_params(L.ACTOR, st.actor)
    eng.set_params(L.CRITIC, st.critic)
    eng.set_params(L.CRITIC_TARGET, st.critic_target)
    eng.set_params(L.LOG_ALPHA, st.log_alpha)


# ---------------------------------------------------------------------------- the solve alone
def _test_matrix(T, P):
    """The matrix of test_gpu_pcgrad.py (mixed magnitudes, zero columns, tiny entries) with the row norms
    spread over 0.05 .. 20: CAGrad clips some rows and leaves others."""
    rng = np.random.default_rng(T)
    G = rng.standard_normal((T, P)) * rng.choice([1e-4, 1e-2, 1.0, 3.0], size=(T, P))
    G[:, rng.choice(P, P // 7, replace=False)] = 0.0
    G *= (rng.permutation(np.geomspace(0.05, 20.0, T)) / np.linalg.norm(G, axis=1))[:, None]
    G = G.astype(np.float32)
    G[0, :4] = [np.float32(1e-30), np.float32(-1e-30), 2.0 * G[0, 2], -2.0 * G[0, 3]]
    return G


def _check_solve(got_w, got, want_w, want, cosine):
    np.testing.assert_allclose(got_w, want_w, rtol=1e-6)
    np.testing.assert_allclose(got["task_weights"], want["task_weights"], rtol=1e-6)
    assert got["best_iteration"] == want["best_iteration"]
    for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery", "avg_cosine_similarity",
              "cagrad_objective", "grad_magnitude"):
        if np.isnan(want[k]):
            assert not cosine and np.isnan(got[k]), k
        else:
            assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])
    hist_err = np.abs(got["obj_hist"] - want["obj_hist"]).max() / np.abs(want["obj_hist"]).max()
    print("obj_hist", hist_err)
    assert hist_err <= HIST_RTOL, hist_err


@pytest.mark.parametrize("which", [0, 1], ids=["critic", "actor"])
@pytest.mark.parametrize("T", [2, 3, 10, 33, 50, 64])
def test_solve_alone(T, which):
    from mtrl_amd.cagrad import cagrad_from_gram

    # T = 2 .. 10: the first row half of the Gram tiles only; 33, 50: both; 64: a full wave, no idle lane
    W = 64 if T == 10 else 32
    e = _engine(T, W, 2)
    P = e.task_gradient_size(which)
    G = _test_matrix(T, P)
    nrm = np.linalg.norm(G.astype(np.float64), axis=1)
    assert (nrm > 1.0).any() and (nrm < 1.0).any()
    e.set_task_gradients(which, G)
    gram = e.task_gram(which)
    for cosine in (False, True):
        # the reference's start: the degenerate search
        w, logs = e.task_cagrad_solve(which, cosine_sim_logs=cosine)
        w_ref, ref = cagrad_from_gram(gram, cosine_sim_logs=cosine)
        assert ref["best_iteration"] == 0
        _check_solve(w, logs, w_ref, ref, cosine)
        np.testing.assert_array_equal(logs["task_weights"], np.full(T, 1.0 / T, np.float32))
        # w0 = 1: a search that moves (the condition of test_cagrad_cpu.py, on the host statement)
        w1, logs1 = e.task_cagrad_solve(which, w0=np.ones(T), cosine_sim_logs=cosine)
        w1_ref, ref1 = cagrad_from_gram(gram, w0=np.ones(T), cosine_sim_logs=cosine)
        tw = ref1["task_weights"]
        assert ref1["best_iteration"] > 0 and tw.max() / tw.min() > 1.5
        _check_solve(w1, logs1, w1_ref, ref1, cosine)
    # other hyperparameters reach the kernel
    w2, logs2 = e.task_cagrad_solve(which, c=0.3, num_iterations=7, learning_rate=3.0, momentum=0.25, w0=np.ones(T))
    w2_ref, ref2 = cagrad_from_gram(gram, c=0.3, num_iterations=7, learning_rate=3.0, momentum=0.25, w0=np.ones(T))
    assert logs2["obj_hist"].shape == (7,)
    _check_solve(w2, logs2, w2_ref, ref2, False)
    # combine with the returned weights: the fp32 ordered sum, through the padded gradient buffer and back
    acc = np.zeros(P, np.float32)
    for t in range(T):
        acc = acc + w1[t] * G[t]
    out = e.task_combine(which, w1)
    ulp = np.spacing(np.abs(acc))
    assert np.all(np.abs(out.astype(np.float64) - acc.astype(np.float64)) <= 2 * ulp)
    e.close()


# ---------------------------------------------------------------------------- the step against the oracle
STEP_CASES = {"t3": (3, 32, 4, 23), "t5": (5, 64, 8, 23), "t10": (10, 128, 16, 32)}  # test_gpu_pcgrad.py's


def _noise(rng, n, T):
    # one (n, A) draw shared by the tasks: rows i*T + t see draw i (the reference's vmap key)
    return np.repeat(rng.standard_normal((n, 4)), T, axis=0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle_run(T, W, n, seed, nsteps):
    """Oracle steps, computed once per shape and shared by the precisions (never mutated)."""
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, seed, head_bound=1.0)
    st0 = st.copy()
    rng = np.random.default_rng(seed + 7)
    steps = []
    for step in range(nsteps):
        batch = synthetic_batch(T, n * T, seed=seed + 100 + step, dtype=np.float32)
        en, ec = _noise(rng, n, T), _noise(rng, n, T)
        st, logs = co.update(cfg, st, batch, en.astype(np.float64), ec.astype(np.float64))
        steps.append((batch, en, ec, logs))
    return cfg, st0, st, steps


def _run_and_compare(T, W, n, seed, nsteps, precision):
    from mtrl_amd import _lib as L

    cfg, st0, st, steps = _oracle_run(T, W, n, seed, nsteps)
    eng = _engine(T, W, n, precision, capacity=256, actor_max_grad_norm=cfg.actor_max_grad_norm,
                  critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_cagrad(True)
    _load_state(eng, st0)
    for step, (batch, en, ec, want) in enumerate(steps):
        eng.update(batch, en, ec)
        got, got_ca = eng.logs(), eng.cagrad_logs()
        print(T, precision, step, {k: (got[k], want[k]) for k in got},
              {k: (got_ca[k], want[k]) for k in got_ca if "task_weights" not in k})
        for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values",
                  "metrics/explore_loss"):
            if k == "losses/alpha_loss" and step == 0:
                assert abs(got[k]) < 1e-6  # log_alpha = 0 at init
                continue
            scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
            assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (step, k, got[k], want[k])
        for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
                  "metrics/actor_params_norm", "alpha"):
            assert abs(got[k] - want[k]) < NORM_RTOL * abs(want[k]), (step, k, got[k], want[k])
        for net in ("critic", "actor"):
            for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery", "cagrad_objective"):
                g, w_ = got_ca[f"metrics/{net}_{k}"], want[f"metrics/{net}_{k}"]
                assert abs(g - w_) <= NORM_RTOL * abs(w_), (step, net, k, g, w_)
            assert np.isnan(got_ca[f"metrics/{net}_avg_cosine_similarity"])
            tw = got_ca[f"metrics/{net}_task_weights"]
            assert tw.dtype == np.float32 and tw.shape == (T,)
            np.testing.assert_array_equal(tw, np.full(T, 1.0 / T, np.float32))
            np.testing.assert_array_equal(want[f"metrics/{net}_task_weights"], np.full(T, 1.0 / T))
    for which, ref in ((L.ACTOR, st.actor), (L.CRITIC, st.critic), (L.CRITIC_TARGET, st.critic_target),
                       (L.LOG_ALPHA, st.log_alpha), (L.ACTOR_ADAM_MU, st.actor_opt.mu),
                       (L.CRITIC_ADAM_MU, st.critic_opt.mu), (L.ACTOR_ADAM_NU, st.actor_opt.nu),
                       (L.CRITIC_ADAM_NU, st.critic_opt.nu)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (which, np.median(d))
        assert d.max() < 2 * 3e-4 * nsteps + 1e-6, (which, d.max())
    assert [eng.get_adam_count(i) for i in range(3)] == [nsteps] * 3
    eng.close()


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_cagrad_step_matches_oracle(name, precision):
    _run_and_compare(*STEP_CASES[name], 3, precision)


def test_cagrad_step_mt50():
    """T = 50 (both row halves of the Gram tiles, learning rate 50): one step, compared in full."""
    _run_and_compare(50, 32, 2, 23, 1, 1)


def test_cagrad_step_cosine_logs_match_oracle():
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, steps = _oracle_run(T, W, n, seed, 3)
    batch, en, ec, _ = steps[0]
    _, want = co.update(cfg, st0, batch, en.astype(np.float64), ec.astype(np.float64), cosine_sim_logs=True)
    eng = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_cagrad(True, cosine_sim_logs=True)
    _load_state(eng, st0)
    eng.update(batch, en, ec)
    got = eng.cagrad_logs()
    for net in ("critic", "actor"):
        k = f"metrics/{net}_avg_cosine_similarity"
        assert abs(got[k] - want[k]) <= NORM_RTOL * abs(want[k]), (k, got[k], want[k])
    eng.close()


# ---------------------------------------------------------------------------- device path
def _snapshot(e):
    return e.logs(), e.cagrad_logs(), [e.get_params(w) for w in range(10)]


def _assert_same(x, y):
    assert x[0] == y[0]
    np.testing.assert_equal(x[1], y[1])
    for a, b in zip(x[2], y[2]):
        np.testing.assert_array_equal(a, b)


def test_update_many_equals_single_device_batch_updates():
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, _ = _oracle_run(T, W, n, seed, 3)

    def make():
        e = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
        e.set_cagrad(True)
        _load_state(e, st0)
        e.buffer_fill_synthetic(7)
        e.seed_rng(1)
        return e

    a, b = make(), make()
    a.update_many(3)
    for _ in range(3):
        b.update()  # device batch, device noise
    sa, sb = _snapshot(a), _snapshot(b)
    _assert_same(sa, sb)
    assert all(np.isfinite(v) for k, v in sa[0].items())
    assert [a.get_adam_count(i) for i in range(3)] == [3, 3, 3]
    for net in ("critic", "actor"):
        np.testing.assert_array_equal(sa[1][f"metrics/{net}_task_weights"], np.full(T, 1.0 / T, np.float32))
    a.close()
    b.close()


# ---------------------------------------------------------------------------- contracts
def test_contracts():
    from mtrl_amd._lib import MTSACError
    from mtrl_amd.engine import MTSACEngine, make_config

    sh = MTSACEngine(make_config(num_tasks=4, task_begin=2, task_count=2, obs_dim=43, actor_width=32, critic_width=32,
                                 batch_per_task=4, capacity=64, precision=1))
    with pytest.raises(MTSACError, match="-95"):
        sh.set_cagrad(True)
    sh.close()
    tw = _engine(3, 32, 4, use_task_weights=1)
    with pytest.raises(MTSACError, match="-95"):
        tw.set_cagrad(True)
    tw.close()
    e = _engine(3, 32, 4)
    for bad in (dict(num_iterations=0), dict(c=-0.1), dict(c=float("nan")), dict(c=float("inf")),
                dict(learning_rate=float("inf")), dict(momentum=float("nan"))):
        with pytest.raises(MTSACError, match="-22"):
            e.set_cagrad(True, **bad)
    e.enable_graph(True)  # nothing above switched the mode on
    e.set_cagrad(True)
    with pytest.raises(MTSACError, match="-95"):
        e.enable_graph(True)
    e.enable_graph(False)
    with pytest.raises(MTSACError, match="-16"):
        e.set_pcgrad(True)
    e.set_cagrad(False)
    e.enable_graph(True)
    e.set_pcgrad(True)
    with pytest.raises(MTSACError, match="-16"):
        e.set_cagrad(True)
    e.set_pcgrad(False)
    e.set_cagrad(True)
    e.set_cagrad(False)
    e.close()


@pytest.mark.parametrize("mode", ["plain", "pcgrad"])
def test_other_steps_untouched_after_a_toggle(mode):
    """An engine that had CAGrad on and off again takes the plain step, and the PCGrad step, bit for bit
    like one that never heard of it."""
    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, 3, head_bound=1.0 if mode == "pcgrad" else 1e-3)
    outs = []
    for touch in (False, True):
        e = _engine(T, W, n, 1)
        if touch:
            e.set_cagrad(True, cosine_sim_logs=True)
            e.set_cagrad(False)
        if mode == "pcgrad":
            e.set_pcgrad(True)
            e.pcgrad_set_order([2, 0, 1], [1, 2, 0])
        _load_state(e, st)
        for step in range(2):
            batch = synthetic_batch(T, n * T, seed=50 + step, dtype=np.float32)
            en, ec = synthetic_eps(n * T, seed=60 + step, dtype=np.float32)
            e.update(batch, en, ec)
        if mode == "pcgrad":
            e.pcgrad_set_order(None, None)
        e.buffer_fill_synthetic(5)
        e.seed_rng(2)
        e.update_many(2)
        outs.append((e.logs(), e.pcgrad_logs() if mode == "pcgrad" else {}, [e.get_params(w) for w in range(10)]))
        e.close()
    _assert_same(outs[0], outs[1])


# ---------------------------------------------------------------------------- trainer
def _algo(T, actor_opt, critic_opt):
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import VanillaNetworkConfig
    from mtrl.rl.algorithms import MTSACConfig

    return MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=VanillaNetworkConfig(width=32, optimizer=actor_opt)),
        critic_config=QValueFunctionConfig(network_config=VanillaNetworkConfig(width=32, optimizer=critic_opt)),
        num_critics=2)


def test_trainer_with_cagrad_on_both_networks():
    from fake_env import FakeMetaworldConfig, FakeMTVecEnv
    from mtrl.config.optim import CAGradConfig, OptimizerConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    T = 3

    class ThreeTasks(FakeMetaworldConfig):  # MetaworldConfig's spaces with three one-hot task columns
        @property
        def num_tasks(self) -> int:
            return T

    plain = OptimizerConfig(max_grad_norm=1.0)
    opt = CAGradConfig(num_tasks=T, max_grad_norm=1.0, cagrad_optimizer=plain)
    env_cfg = ThreeTasks(env_id="MT3")
    assert env_cfg.observation_space.shape == (39 + T,)
    with pytest.raises(NotImplementedError, match="one network only"):
        MTSAC.initialize(_algo(T, opt, plain), env_cfg, seed=1)
    tc = OffPolicyTrainingConfig(total_steps=1000, buffer_size=50 * T, batch_size=8 * T, warmstart_steps=5,
                                 evaluation_frequency=10)
    agent = MTSAC.initialize(_algo(T, opt, opt), env_cfg, seed=1, precision="split3")
    assert agent.cagrad and not agent.pcgrad
    buf = agent.spawn_replay_buffer(env_cfg, tc, 1)
    env = FakeMTVecEnv(T)
    obs, _ = env.reset()
    for _ in range(12):
        nobs, r, term, trunc, _ = env.step(env.action_space.sample())
        buf.add(obs, nobs, env.action_space.sample(), r, np.logical_or(term, trunc))
        obs = nobs
    for _ in range(3):
        agent, logs = agent.update_from_buffer(buf, tc.batch_size, want_logs=True)
        d = dict(logs)
        assert len(logs) == len(d) == 20
        for net in ("critic", "actor"):
            tw = d[f"metrics/{net}_task_weights"]
            assert tw.shape == (T,) and np.all(np.isfinite(tw)) and abs(tw.sum() - 1.0) < 1e-6
            assert np.isnan(d[f"metrics/{net}_avg_cosine_similarity"])
            for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery", "cagrad_objective"):
                assert np.isfinite(d[f"metrics/{net}_{k}"]), k
        assert all(np.isfinite(v) for k, v in d.items() if np.ndim(v) == 0 and "cosine" not in k)
    assert {f"metrics/{net}_{k}" for net in ("critic", "actor") for k in co.CA_KEYS} <= set(d)
    assert agent.engine.get_adam_count(0) == 3 and agent.engine.get_adam_count(1) == 3
