"""Per-task batch sizes through the drop-in surface: MultiTaskReplayBuffer.sample with an array, and the trainer
with TrainingConfig.sampler_type on the synthetic vector env of tests/test_gpu_trainer.py."""

from __future__ import annotations

import numpy as np
import pytest

import task_batch_cases as tc

pytestmark = pytest.mark.gpu


def test_buffer_sample_with_an_array_of_sizes():
    from mtrl_amd.compat.rl.buffers import MultiTaskReplayBuffer
    from mtrl_amd.compat.types import ReplayBufferSamples
    from mtrl_amd.engine import MTSACEngine, make_config

    name, sizes = "t3", np.array([1, 0, 23])
    T, n, W, A, E = tc.SHAPES[name]
    B = n * T
    eng = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, action_dim=A, actor_width=W, critic_width=W,
                                  num_critics=E, batch_per_task=n, capacity=tc.CAPACITY, normalize_rewards=1))
    buf = MultiTaskReplayBuffer(tc.CAPACITY * T, T, seed=5, normalize_rewards=True, engine=eng)
    store = tc.make_store(T, A, tc.CAPACITY, seed=8)
    tc.fill_engine(eng, store)
    eng.set_reward_stats(np.full(T, -2.0), np.full(T, 12.0))
    rng = np.random.default_rng(5)  # the buffer seeded the device stream like default_rng(seed)
    for s in (sizes, np.array([9, 8, 7])):
        got = buf.sample(s)
        assert isinstance(got, ReplayBufferSamples)
        _, (obs, act, nobs, done, rew, _) = tc.reference_sample(store, rng, s, tc.CAPACITY, B)
        for g, w in zip(got, (obs, act, nobs, done, rew)):  # the array branch returns raw rewards
            np.testing.assert_array_equal(np.asarray(g), w)
        assert eng.task_batch_sizes().tolist() == s.tolist()
    with pytest.raises(AssertionError):
        buf.sample(np.array([12, 12]))
    with pytest.raises(AssertionError):
        buf.sample(np.array([9, 8, 8]))
    assert eng.task_batch_sizes().tolist() == [9, 8, 7]  # a refused call changes nothing
    # an int: the sizes are cleared, rows interleaved, rewards normalised
    got = buf.sample(B)
    assert not eng.task_batch_sizes_set()
    i = rng.integers(0, tc.CAPACITY, size=n)
    np.testing.assert_array_equal(got.observations, store[0][i].reshape(B, -1))
    want_r = ((store[3][i].astype(np.float64) + 2.0) / (12.0 + 2.0 + 1e-8)).astype(np.float32).reshape(B, 1)
    np.testing.assert_array_equal(got.rewards, want_r)
    assert eng.get_rng_state() == rng.bit_generator.state
    eng.close()


def _experiment(tmp_path, T, total, **training):
    from fake_env import FakeMetaworldConfig
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.experiment import Experiment
    from mtrl.rl.algorithms import MTSACConfig

    return Experiment(
        exp_name="fake_sampler", seed=1, data_dir=tmp_path, env=FakeMetaworldConfig(env_id="MT10"),
        algorithm=MTSACConfig(
            num_tasks=T, gamma=0.99,
            actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(
                num_tasks=T, width=64, optimizer=OptimizerConfig(max_grad_norm=1.0))),
            critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(
                num_tasks=T, width=64, optimizer=OptimizerConfig(max_grad_norm=1.0))),
            num_critics=2),
        training_config=OffPolicyTrainingConfig(total_steps=total, buffer_size=200 * T, batch_size=16 * T,
                                                warmstart_steps=20, evaluation_frequency=10, **training),
        checkpoint=False)


def _tensors(agent):
    return [agent.engine.get_params(w) for w in range(10)]


@pytest.mark.parametrize("kind", ["loss", "adaptive"])
def test_trainer_with_a_sampler(tmp_path, kind):
    """45 steps on 10 tasks, 24 gradient steps, new sizes every 3 of them: they change, sum to the batch, are
    logged, and survive the evaluation's balanced metrics sample (evaluation_frequency = 10 episodes, episodes of
    7 steps)."""
    from fake_env import FakeMTVecEnv

    T = 10
    B = 16 * T
    agent = _experiment(tmp_path, T, T * 45, sampler_type=kind, update_weights_every=3).run(envs=FakeMTVecEnv(T, max_steps=7))
    steps = 45 - 21
    assert agent.engine.get_adam_count(0) == steps
    hist = agent.sampler_log_history
    assert len(hist) == steps // 3
    for logs in hist:
        assert sorted(logs) == sorted(f"sampler/batch_size_task_{t}" for t in range(T))
        assert sum(logs.values()) == B and min(logs.values()) >= 0
    assert any(v != 16 for v in hist[0].values()), "the sizes must move off the balanced 16 per task"
    if kind == "loss":  # proportional to the losses: they keep moving (the softmax of an EMA from ones may hold a
        # pattern of 15 / 16 / 17 for a while)
        assert len({tuple(sorted(h.items())) for h in hist}) > 1
    assert agent.engine.task_batch_sizes_set()
    assert agent.engine.task_batch_sizes().tolist() == [hist[-1][f"sampler/batch_size_task_{t}"] for t in range(T)]
    assert all(np.isfinite(v) for v in agent.engine.logs().values())
    assert np.all(np.isfinite(agent.engine.task_losses()))


def test_trainer_without_a_sampler_is_unchanged(tmp_path):
    """sampler_type=None is the run without the field, bit for bit, and leaves the loss reduction off."""
    from fake_env import FakeMTVecEnv
    from mtrl_amd import _lib as L

    T = 10
    a = _experiment(tmp_path / "a", T, T * 30).run(envs=FakeMTVecEnv(T, max_steps=7))
    b = _experiment(tmp_path / "b", T, T * 30, sampler_type=None).run(envs=FakeMTVecEnv(T, max_steps=7))
    for x, y in zip(_tensors(a), _tensors(b)):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a.engine.logs() == b.engine.logs() and a.sampler_log_history == b.sampler_log_history == []
    for agent in (a, b):
        assert not agent.engine.task_batch_sizes_set()
        with pytest.raises(L.MTSACError, match="-22"):
            agent.engine.task_losses()


def test_trainer_refuses_a_sampler_with_gradient_surgery(tmp_path):
    from fake_env import FakeMetaworldConfig
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import PCGradConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.rl.algorithms import MTSACConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    T = 10
    opt = PCGradConfig(num_tasks=T, max_grad_norm=1.0)
    algo = MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=opt)),
        critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=opt)))
    agent = MTSAC.initialize(algo, FakeMetaworldConfig(env_id="MT10"), seed=1)
    assert agent.pcgrad
    with pytest.raises(NotImplementedError, match="PCGrad"):
        agent.setup_task_sampler(OffPolicyTrainingConfig(total_steps=10, sampler_type="loss"))
    agent.setup_task_sampler(OffPolicyTrainingConfig(total_steps=10))
    agent.engine.close()
