"""PCGrad on the CPU: the Gram-form solve (mtrl_amd/pcgrad.py) against the literal sequential
projection, and the config surface (mtrl.config.optim.PCGradConfig, MTSAC.initialize's refusals)."""

from __future__ import annotations

import numpy as np
import pytest


def _matrix(T, P, kind, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((T, P)) * rng.choice([1e-2, 1.0, 3.0], size=(T, 1))
    if kind == "orthogonal":  # rows 0 and 1 exactly orthogonal (disjoint supports)
        M[0, P // 2:] = 0.0
        M[1, :P // 2] = 0.0
    elif kind == "zero_row":
        M[T - 1] = 0.0
    return M


@pytest.mark.parametrize("kind", ["random", "orthogonal", "zero_row"])
@pytest.mark.parametrize("T", [2, 3, 10, 50])
def test_gram_form_matches_direct_projection(T, kind):
    from mtrl_amd.pcgrad import pcgrad_direct, pcgrad_from_gram

    P = 4 * T + 7
    M = _matrix(T, P, kind, seed=T)
    perm = np.random.default_rng(T + 1).permutation(T)
    if kind == "orthogonal":
        assert (M @ M.T)[0, 1] == 0.0
    w, logs = pcgrad_from_gram(M @ M.T, perm, cosine_sim_logs=True)
    want, want_logs = pcgrad_direct(M, perm, cosine_sim_logs=True)
    got = w @ M
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    assert logs["n_grad_conflicts"] == want_logs["n_grad_conflicts"]
    if kind == "random" and T >= 3:
        assert logs["n_grad_conflicts"] > 0  # the projections are exercised
    for k, v in want_logs.items():
        assert abs(logs[k] - v) <= 1e-12 * max(abs(v), 1.0), (k, logs[k], v)
    w0, logs0 = pcgrad_from_gram(M @ M.T, perm)
    np.testing.assert_array_equal(w0, w)
    assert np.isnan(logs0["avg_cosine_similarity"]) and np.isnan(logs0["avg_cosine_similarity_diff"])


def test_order_does_not_matter_without_conflicts():
    from mtrl_amd.pcgrad import pcgrad_from_gram

    T = 6
    M = np.abs(_matrix(T, 40, "random", seed=3))  # every pair has a positive dot product
    G = M @ M.T
    w, logs = pcgrad_from_gram(G)
    assert logs["n_grad_conflicts"] == 0
    np.testing.assert_array_equal(w, np.full(T, 1.0 / T))
    for s in range(3):
        w2, logs2 = pcgrad_from_gram(G, np.random.default_rng(s).permutation(T))
        np.testing.assert_array_equal(w2, w)
        assert logs2["n_grad_conflicts"] == 0
        assert abs(logs2["grad_magnitude"] - logs["grad_magnitude"]) <= 1e-15 * logs["grad_magnitude"]


def test_order_matters_with_conflicts():
    from mtrl_amd.pcgrad import pcgrad_from_gram

    M = np.array([[1.0, 0.0, 0.2], [-0.8, 0.6, 0.1], [0.1, -0.9, 0.3]])
    w1, _ = pcgrad_from_gram(M @ M.T, [0, 1, 2])
    w2, _ = pcgrad_from_gram(M @ M.T, [2, 1, 0])
    assert np.abs(w1 - w2).max() > 1e-3


def _algo(actor_opt, critic_opt, T=3, **kw):
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.rl.algorithms import MTSACConfig

    return MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=actor_opt)),
        critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=critic_opt)),
        num_critics=2, **kw)


def test_pcgrad_config_surface():
    from mtrl.config.optim import OptimizerConfig, PCGradConfig

    c = PCGradConfig(num_tasks=10, max_grad_norm=1.0)
    assert isinstance(c, OptimizerConfig)
    assert c.requires_split_task_losses is True and c.cosine_sim_logs is False
    assert (c.num_tasks, c.max_grad_norm, c.adam_eps) == (10, 1.0, 1e-5)
    assert PCGradConfig(num_tasks=3, cosine_sim_logs=True).cosine_sim_logs is True
    assert OptimizerConfig().requires_split_task_losses is False


def test_initialize_refuses_unsupported_pcgrad_combinations():
    """Raised before any engine is created (no device call)."""
    from fake_env import FakeMetaworldConfig
    from mtrl.config.optim import OptimizerConfig, PCGradConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    env = FakeMetaworldConfig(env_id="MT10")
    T = 10
    pc, plain = PCGradConfig(num_tasks=T, max_grad_norm=1.0), OptimizerConfig(max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="one network only"):
        MTSAC.initialize(_algo(pc, plain, T), env, seed=1)
    with pytest.raises(NotImplementedError, match="one network only"):
        MTSAC.initialize(_algo(plain, pc, T), env, seed=1)
    with pytest.raises(NotImplementedError, match="use_task_weights"):
        MTSAC.initialize(_algo(pc, pc, T, use_task_weights=True), env, seed=1)
    with pytest.raises(NotImplementedError, match="sharded"):
        MTSAC.initialize(_algo(pc, pc, T), env, seed=1, task_shard=(0, 5))
