"""Per-task batch sizes, the parts that need no GPU: the two samplers of mtrl_amd/compat/rl/sampling_algs.py
against hand-computed sizes, the buffer's argument checks, the trainer's refusals, the new ABI symbols, and the
reference's array-branch arithmetic (tests/task_batch_cases.py) on every size vector the GPU tests use."""

from __future__ import annotations

import pathlib
import re
import types

import numpy as np
import pytest

import task_batch_cases as tc

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mtsac_set_task_batch_sizes", "mtsac_get_task_batch_sizes", "mtsac_set_task_loss_logging",
               "mtsac_get_task_losses", "mtsac_debug_replay_indices_tasks")


# ------------------------------------------------------------------ samplers
def test_sampler_sizes_by_hand():
    from mtrl_amd.compat.rl.sampling_algs import Sampler

    s = Sampler()
    # weights 1/4, 1/4, 1/2: exact, no remainder
    np.testing.assert_array_equal(s.sample_batch_sizes(np.array([1.0, 1.0, 2.0]), 24), [6, 6, 12])
    # all equal: 20 / 3 = 6.67 truncates to 6 each, the remainder 2 goes to the FIRST two tasks
    np.testing.assert_array_equal(s.sample_batch_sizes(np.array([1.0, 1.0, 1.0]), 20), [7, 7, 6])
    # 24 * (1, 2, 4) / 7 = 3.43, 6.86, 13.71 -> 3, 6, 13; remainder 2 to tasks 0 and 1, the SMALLEST losses
    np.testing.assert_array_equal(s.sample_batch_sizes(np.array([1.0, 2.0, 4.0]), 24), [4, 7, 13])
    # astype(int) truncates toward zero: 9.99 -> 9 (not 10)
    np.testing.assert_array_equal(s.sample_batch_sizes(np.array([999.0, 1.0]), 10), [10, 0])  # 9.99 -> 9 + 1, 0.01 -> 0
    # float32 losses as the engine returns them
    out = s.sample_batch_sizes(np.array([0.5, 0.25, 0.25], np.float32), 24)
    np.testing.assert_array_equal(out, [12, 6, 6])
    assert np.issubdtype(out.dtype, np.integer)


def test_adaptive_sampler_sizes_by_hand():
    from mtrl_amd.compat.rl.sampling_algs import AdaptiveSampler

    a = AdaptiveSampler(3)
    # EMA from ones stays ones; softmax 1/3 each; 20 / 3 -> 6 each; the remainder 2 goes to the top of a stable
    # ascending argsort, which among equal weights are the LAST two tasks
    np.testing.assert_array_equal(a.sample_batch_sizes(np.ones(3), 20), [6, 7, 7])
    np.testing.assert_array_equal(a.task_losses_ema, np.ones(3, np.float32))
    # EMA 0.1 * (11, 1, 1) + 0.9 * 1 = (2, 1, 1); softmax = (e^2, e, e) / (e^2 + 2 e) = 0.5761, 0.2119, 0.2119;
    # times 24 = 13.83, 5.09, 5.09 -> 13, 5, 5; remainder 1 to the top weight, task 0
    a = AdaptiveSampler(3)
    np.testing.assert_array_equal(a.sample_batch_sizes(np.array([11.0, 1.0, 1.0]), 24), [14, 5, 5])
    np.testing.assert_allclose(a.task_losses_ema, [2.0, 1.0, 1.0], rtol=1e-6)
    np.testing.assert_allclose(a.get_sampling_weights(), np.exp([2.0, 1, 1]) / np.exp([2.0, 1, 1]).sum(), rtol=1e-6)
    # the state carries: a second call moves the EMA again, 0.1 * 1 + 0.9 * 2 = 1.9
    a.sample_batch_sizes(np.ones(3), 24)
    np.testing.assert_allclose(a.task_losses_ema, [1.9, 1.0, 1.0], rtol=1e-6)
    # temperature and ema_alpha are read
    b = AdaptiveSampler(2, ema_alpha=1.0, temperature=2.0)
    b.update(np.array([2.0, 0.0]))
    np.testing.assert_allclose(b.get_sampling_weights(), np.exp([1.0, 0]) / np.exp([1.0, 0]).sum(), rtol=1e-6)


@pytest.mark.parametrize("kind", ["loss", "adaptive"])
def test_sampler_sizes_sum_to_the_batch(kind):
    from mtrl_amd.compat.rl.sampling_algs import make_sampler

    rng = np.random.default_rng(3)
    for T, B in ((1, 5), (3, 24), (4, 20), (10, 1280), (50, 6400)):
        s = make_sampler(kind, T)
        for _ in range(20):
            losses = rng.uniform(1e-3, 30.0, T).astype(np.float32)
            sizes = s.sample_batch_sizes(losses, B)
            assert sizes.shape == (T,) and sizes.sum() == B and sizes.min() >= 0, (kind, T, losses, sizes)
        eq = make_sampler(kind, T).sample_batch_sizes(np.full(T, 0.7, np.float32), B)
        assert eq.sum() == B and eq.max() - eq.min() <= 1


def test_make_sampler_kinds():
    from mtrl_amd.compat.rl.sampling_algs import AdaptiveSampler, Sampler, make_sampler

    assert make_sampler(None, 3) is None
    assert isinstance(make_sampler("loss", 3), Sampler) and isinstance(make_sampler("adaptive", 3), AdaptiveSampler)
    with pytest.raises(ValueError):
        make_sampler("softmax", 3)


# ------------------------------------------------------------------ the reference arithmetic on every case
def test_reference_arithmetic_accepts_every_case():
    """buffers.py:496-519 in numpy takes every size vector of the GPU tests, from a full and a partly filled
    buffer: B rows, task-major, each row its task's record at its index.  No case is skipped."""
    ran = 0
    for name, sizes in tc.CASES:
        T, n, W, A, E = tc.SHAPES[name]
        assert len(sizes) == T and sum(sizes) == n * T and max(sizes) <= tc.CAPACITY
        store = tc.make_store(T, A, tc.CAPACITY, seed=1)
        for buffer_size in (tc.CAPACITY, 5):
            idx, (obs, act, nobs, done, rew, task) = tc.reference_sample(store, np.random.default_rng(7), sizes,
                                                                         buffer_size, n * T)
            assert obs.shape == (n * T, 39 + T) and act.shape == (n * T, A) and rew.shape == done.shape == (n * T, 1)
            np.testing.assert_array_equal(task, np.repeat(np.arange(T), sizes))
            np.testing.assert_array_equal(np.argmax(obs[:, 39:], axis=1), task)
            for t in range(T):
                assert len(idx[t]) == sizes[t]
                assert np.all(idx[t] < max(buffer_size, sizes[t]))
            ran += 1
    assert ran == 2 * len(tc.CASES) == 14
    with pytest.raises(AssertionError):
        tc.reference_sample(store, np.random.default_rng(7), (7, 6, 4, 4), tc.CAPACITY, 20)


# ------------------------------------------------------------------ buffer argument checks
class _StubEngine:
    """What MultiTaskReplayBuffer touches, without a device."""

    def __init__(self, T, n):
        self.config = types.SimpleNamespace(batch_per_task=n, normalize_rewards=0)
        self.T_l, self.B = T, n * T
        self.sizes, self.calls = None, []

    def seed_rng(self, seed):
        pass

    def task_batch_sizes_set(self):
        return self.sizes is not None

    def set_task_batch_sizes(self, sizes):
        self.sizes = None if sizes is None else np.asarray(sizes).copy()
        self.calls.append(self.sizes)

    def sample(self):
        B = self.B
        z = np.zeros((B, 1), np.float32)
        return np.zeros(B if self.sizes is not None else B // self.T_l, np.int64), (z, z, z, z, z)


def test_buffer_sample_argument_checks():
    from mtrl_amd.compat.rl.buffers import MultiTaskReplayBuffer

    T, n = 3, 8
    eng = _StubEngine(T, n)
    buf = MultiTaskReplayBuffer(64 * T, T, seed=1, engine=eng)
    with pytest.raises(AssertionError):
        buf.sample(np.array([12, 12]))  # wrong length
    with pytest.raises(AssertionError):
        buf.sample(np.array([9, 8, 8]))  # wrong sum
    with pytest.raises(AssertionError):
        buf.sample(25)  # not a multiple of T
    assert eng.calls == []
    buf.sample(np.array([9, 8, 7]))
    np.testing.assert_array_equal(eng.sizes, [9, 8, 7])
    buf.sample(np.array([24, 0, 0]))  # the sizes stay set between array calls
    np.testing.assert_array_equal(eng.sizes, [24, 0, 0])
    buf.sample(24)  # an int clears them first
    assert eng.sizes is None and len(eng.calls) == 3
    buf.sample(np.int64(24))  # and a numpy integer is an int, not an array of sizes
    assert len(eng.calls) == 3


# ------------------------------------------------------------------ the trainer's refusals
def _bare_agent(T, surgery=None, T_l=None):
    from mtrl_amd.compat.rl.algorithms.mtsac import MTSAC

    agent = MTSAC.__new__(MTSAC)
    agent.num_tasks, agent.surgery = T, surgery
    agent.sampler_log_history = []
    calls = []
    agent.engine = types.SimpleNamespace(T_l=T if T_l is None else T_l, B=8 * T,
                                         set_task_loss_logging=lambda on: calls.append(on))
    return agent, calls


def test_trainer_refuses_what_cannot_run():
    from mtrl_amd.compat.config.rl import OffPolicyTrainingConfig
    from mtrl_amd.compat.rl.algorithms.base import OffPolicyAlgorithm

    cfg = OffPolicyTrainingConfig(total_steps=10, sampler_type="loss", update_weights_every=3)
    for mode in ("pcgrad", "cagrad", "gradnorm"):
        agent, calls = _bare_agent(3, surgery=mode)
        with pytest.raises(NotImplementedError, match="interleaved rows"):
            agent.setup_task_sampler(cfg)
        assert calls == []
    agent, calls = _bare_agent(4, T_l=2)
    with pytest.raises(NotImplementedError, match="task-sharded"):
        agent.setup_task_sampler(cfg)
    agent, calls = _bare_agent(3)
    with pytest.raises(ValueError):
        agent.setup_task_sampler(OffPolicyTrainingConfig(total_steps=10, sampler_type="nope"))
    # an algorithm without the engine support refuses the field, and runs without it
    with pytest.raises(NotImplementedError, match="sampler_type"):
        OffPolicyAlgorithm.setup_task_sampler(agent, cfg)
    OffPolicyAlgorithm.setup_task_sampler(agent, OffPolicyTrainingConfig(total_steps=10))
    # None changes nothing; a sampler turns the per-task loss logging on
    agent.setup_task_sampler(OffPolicyTrainingConfig(total_steps=10))
    assert agent._sampler is None and calls == [] and agent.task_sampler_step() == {}
    agent.setup_task_sampler(cfg)
    assert calls == [True] and agent._sampler_every == 3


def test_trainer_sampler_step_period_and_logs():
    from mtrl_amd.compat.config.rl import OffPolicyTrainingConfig

    T = 3
    agent, _ = _bare_agent(T)
    set_calls = []
    agent.engine.task_losses = lambda: np.array([[1.0, 2.0, 4.0], [9.0, 9.0, 9.0]], np.float32)
    agent.engine.set_task_batch_sizes = lambda s: set_calls.append(np.asarray(s).copy())
    agent.setup_task_sampler(OffPolicyTrainingConfig(total_steps=10, sampler_type="loss", update_weights_every=3))
    out = [agent.task_sampler_step() for _ in range(7)]
    assert [bool(o) for o in out] == [False, False, True, False, False, True, False]
    assert out[2] == {"sampler/batch_size_task_0": 4, "sampler/batch_size_task_1": 7, "sampler/batch_size_task_2": 13}
    assert len(set_calls) == 2 and set_calls[0].tolist() == [4, 7, 13]  # the critic's losses, row 0
    agent.task_sampler_restore()  # after the evaluation's balanced sample
    assert len(set_calls) == 3 and set_calls[2].tolist() == [4, 7, 13]
    assert agent.sampler_log_history == [out[2], out[5]]


# ------------------------------------------------------------------ ABI
def test_new_symbols_are_declared_bound_and_exported():
    from mtrl_amd import _lib

    text = "".join(re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S) for h in (ROOT / "include").glob("*.h"))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    from mtrl_amd.engine import MTSACEngine

    for method in ("set_task_batch_sizes", "task_batch_sizes", "set_task_loss_logging", "task_losses"):
        assert callable(getattr(MTSACEngine, method))
    # null handles are refused before anything touches a device
    assert lib.mtsac_set_task_batch_sizes(None, None) == -22
    assert lib.mtsac_get_task_batch_sizes(None, None) == -22
    assert lib.mtsac_set_task_loss_logging(None, 1) == -22
    assert lib.mtsac_get_task_losses(None, None) == -22
