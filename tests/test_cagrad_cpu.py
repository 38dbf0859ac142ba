"""CAGrad on the CPU: the Gram-form host statement (mtrl_amd/cagrad.py) against the reference's literal
statement with torch.autograd's gradient, the degeneracy of the reference's weight search pinned, the
clip folded into the Gram matrix, and the config surface (mtrl.config.optim.CAGradConfig,
MTSAC.initialize's refusals)."""

from __future__ import annotations

import numpy as np
import pytest

from cagrad_oracle import matrix_families

FAMILIES = ("random", "half_conflicting", "cancelling", "tiny", "zero")
# the families whose objective depends on w beyond rounding: on cancelling rows Gg = GG 1 / T is rounding
# noise, on tiny and zero rows GG itself is <= 1e-14, so from any start the search sees a flat objective,
# never moves to a better iterate and no seed can make it (checked below)
CURVED = ("random", "half_conflicting")
# seeds picked on the CPU (the host statement alone) so that from w0 = 1 the best iterate is not the
# first and max / min task weight > 1.5 with a margin: (T, family) -> seed
SEEDS = {(3, "random"): 9, (10, "random"): 10, (50, "random"): 50,
         (3, "half_conflicting"): 3, (10, "half_conflicting"): 11, (50, "half_conflicting"): 56}


def _family(T, kind, P=200):
    return matrix_families(T, P, SEEDS.get((T, kind), T))[kind]


def _prepared(G, c=0.5):
    from mtrl_amd.cagrad import clip_scales

    s = clip_scales(G)
    Gp = s[:, None] * G * s[None, :]
    GG = Gp / np.sqrt(np.diag(Gp) + 1e-4).mean() ** 2
    Gg = GG.mean(axis=1)
    return GG, Gg, c * np.sqrt(Gg.mean() + 1e-4)


# ---------------------------------------------------------------------------- 1. analytic gradient
@pytest.mark.parametrize("T", [3, 10, 50])
def test_analytic_gradient_matches_autograd(T):
    import torch

    from mtrl_amd.cagrad import objective_and_grad

    GG, Gg, c_n = _prepared((lambda M: M @ M.T)(_family(T, "half_conflicting")))
    rng = np.random.default_rng(T)
    GG_t, Gg_t = torch.from_numpy(GG), torch.from_numpy(Gg)
    checked = 0
    for _ in range(20):
        w = rng.standard_normal(T) * rng.choice([0.1, 1.0, 30.0])
        if abs(w.sum()) <= 0.1:
            continue
        wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        ww = wt / (wt.sum() + 1e-8)
        obj_t = ww @ Gg_t + c_n * torch.sqrt(ww @ GG_t @ ww + 1e-4)
        (g_t,) = torch.autograd.grad(obj_t, wt)
        obj, g = objective_and_grad(w, GG, Gg, c_n)
        assert abs(obj - obj_t.item()) <= 1e-13 * abs(obj_t.item())
        assert np.abs(g - g_t.numpy()).max() <= 1e-12 * np.abs(g_t.numpy()).max(), (w.sum(),)
        checked += 1
    assert checked >= 10


# ---------------------------------------------------------------------------- 2. host form against the literal statement
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _compare(got_g, got_logs, want_g, want_logs):
    """Largest relative difference (each vector against its largest entry) over the combined gradient,
    the logs and obj_hist."""
    worst = max(_rel(got_g, want_g), _rel(got_logs["obj_hist"], want_logs["obj_hist"]),
                _rel(got_logs["task_weights"], want_logs["task_weights"]))
    assert got_logs["best_iteration"] == want_logs["best_iteration"]
    for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery", "avg_cosine_similarity",
              "cagrad_objective", "grad_magnitude"):
        worst = max(worst, _rel(got_logs[k], want_logs[k]))
    return worst


@pytest.mark.parametrize("start", ["reference", "ones"])
@pytest.mark.parametrize("kind", CURVED)
@pytest.mark.parametrize("T", [3, 10, 50])
def test_gram_form_matches_literal_statement(T, kind, start):
    """The bound is 10x the difference between two runs of the literal statement with the task rows in
    forward and in reversed order (a pure reordering of float64 sums), floor 1e-12.  Measured here over
    the twelve cases: reordering 7e-17 .. 2.8e-15, this comparison 2e-16 .. 5.4e-14 (the largest at T = 3,
    half_conflicting, w0 = 1, where max / min task weight is in the hundreds): the floor decides every case."""
    from mtrl_amd.cagrad import cagrad_direct, cagrad_from_gram

    M = _family(T, kind)
    w0 = None if start == "reference" else np.ones(T)
    want_g, want = cagrad_direct(M, w0=w0, cosine_sim_logs=True)
    rev_g, rev = cagrad_direct(M[::-1], w0=w0, cosine_sim_logs=True)
    rev = dict(rev, task_weights=rev["task_weights"][::-1])
    reorder = _compare(rev_g, rev, want_g, want)
    bound = max(10.0 * reorder, 1e-12)
    w, logs = cagrad_from_gram(M @ M.T, w0=w0, cosine_sim_logs=True)
    diff = _compare(w @ M, logs, want_g, want)
    print(T, kind, start, "reorder", reorder, "gram form", diff)
    assert diff <= bound, (diff, bound)
    # without the cosine logs: the same weights, NaN in the log
    w_nc, logs_nc = cagrad_from_gram(M @ M.T, w0=w0)
    np.testing.assert_array_equal(w_nc, w)
    assert np.isnan(logs_nc["avg_cosine_similarity"])


# ---------------------------------------------------------------------------- 3. the degeneracy, pinned
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("T", [3, 10, 50])
def test_reference_search_never_leaves_its_start(T, kind):
    from mtrl_amd.cagrad import cagrad_from_gram

    M = _family(T, kind)
    G = M @ M.T
    w, logs = cagrad_from_gram(G)
    np.testing.assert_array_equal(logs["task_weights"], np.full(T, 1.0 / T))
    assert logs["best_iteration"] == 0
    assert logs["cagrad_objective"] == 0.01 * logs["c_normalized"]
    assert logs["obj_hist"].shape == (21,) and np.all(logs["obj_hist"][1:] >= logs["obj_hist"][0])
    # the update is (1 + lambda) / (1 + c^2) mean_t g'_t
    GG, _, c_n = _prepared(G)
    lam = c_n / (np.sqrt(GG.mean() + 1e-4) + 1e-4)
    nrm = np.linalg.norm(M, axis=1)
    Mc = M * np.minimum(1.0, 1.0 / (nrm + 1e-8))[:, None]
    want = (1.0 + lam) / 1.25 * Mc.mean(axis=0)
    assert np.abs(w @ M - want).max() <= 1e-14 * np.abs(Mc).max()  # (cancelling rows: the mean itself is ~0)
    # from w0 = 1 the search moves: on the families whose objective is not flat
    w1, logs1 = cagrad_from_gram(G, w0=np.ones(T))
    tw = logs1["task_weights"]
    if kind in CURVED:
        assert logs1["best_iteration"] > 0
        assert tw.max() / tw.min() > 1.5, tw.max() / tw.min()
    else:  # flat to rounding: the start stays the best iterate whatever the seed
        for seed in range(5):
            Ms = matrix_families(T, 200, 100 + seed)[kind]
            assert cagrad_from_gram(Ms @ Ms.T, w0=np.ones(T))[1]["best_iteration"] == 0


# ---------------------------------------------------------------------------- 4. clip folded into the Gram
def test_clip_scales_from_the_gram_diagonal():
    from mtrl_amd.cagrad import cagrad_direct, cagrad_from_gram, clip_scales

    rng = np.random.default_rng(0)
    T, P = 6, 50
    M = rng.standard_normal((T, P))
    M *= (np.array([0.01, 0.5, 0.999, 1.001, 3.0, 0.0]) / np.maximum(np.linalg.norm(M, axis=1), 1e-300))[:, None]
    nrm = np.linalg.norm(M, axis=1)
    assert (nrm < 1).sum() >= 3 and (nrm > 1).sum() >= 2 and nrm[-1] == 0.0
    s = clip_scales(M @ M.T)
    want = np.minimum(1.0, 1.0 / (nrm + 1e-8))
    assert np.abs(s - want).max() <= 1e-15
    assert np.all(s[nrm < 0.9] == 1.0) and np.all(s[nrm > 1] < 1.0) and s[-1] == 1.0
    Mc = M * want[:, None]
    Gp = s[:, None] * (M @ M.T) * s[None, :]
    assert np.abs(Gp - Mc @ Mc.T).max() <= 1e-15
    w, logs = cagrad_from_gram(M @ M.T, w0=np.ones(T))
    g, want_logs = cagrad_direct(M, w0=np.ones(T))
    assert np.abs(w @ M - g).max() <= 1e-12 * np.abs(g).max()
    assert np.all(np.isfinite(w)) and w[-1] >= (1.0 / T) / 1.25  # the zero row: s = 1, weight 1/T and up
    assert abs(logs["avg_grad_magnitude_before_surgery"] - np.linalg.norm(Mc, axis=1).mean()) <= 1e-15


# ---------------------------------------------------------------------------- 5. config
def _algo(actor_opt, critic_opt, T=3, **kw):
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import VanillaNetworkConfig
    from mtrl.rl.algorithms import MTSACConfig

    return MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=VanillaNetworkConfig(width=32, optimizer=actor_opt)),
        critic_config=QValueFunctionConfig(network_config=VanillaNetworkConfig(width=32, optimizer=critic_opt)),
        num_critics=2, **kw)


def test_cagrad_config_surface():
    import dataclasses

    from mtrl.config.optim import CAGradConfig, OptimizerConfig
    from mtrl_amd.cagrad import LOG_KEYS
    from mtrl_amd.compat.config import optim as compat_optim
    from mtrl_amd.engine import CAGRAD_LOG_KEYS

    assert CAGradConfig is compat_optim.CAGradConfig
    c = CAGradConfig(num_tasks=10, max_grad_norm=1.0, cagrad_optimizer=OptimizerConfig(max_grad_norm=1.0))
    assert isinstance(c, OptimizerConfig)
    assert c.requires_split_task_losses is True
    assert (c.num_tasks, c.max_grad_norm, c.adam_eps, c.lr, c.initial_weights) == (10, 1.0, 1e-5, 3e-4, None)
    assert dataclasses.replace(c, num_tasks=3) == CAGradConfig(
        num_tasks=3, max_grad_norm=1.0, cagrad_optimizer=OptimizerConfig(max_grad_norm=1.0))
    assert {"num_tasks", "cagrad_optimizer", "initial_weights", "max_grad_norm"} <= {
        f.name for f in dataclasses.fields(c)}
    with pytest.raises(TypeError):
        CAGradConfig(num_tasks=3)  # cagrad_optimizer has no default in the reference either
    assert LOG_KEYS == CAGRAD_LOG_KEYS == ("task_weights", "avg_grad_magnitude", "avg_grad_magnitude_before_surgery",
                                           "avg_cosine_similarity", "cagrad_objective")


def test_experiment_script_imports_resolve():
    """Every name experiments/misc/mt10_mtmhsac_cagrad.py imports from mtrl.*."""
    import importlib

    names = {
        "mtrl.config.networks": ("ContinuousActionPolicyConfig", "QValueFunctionConfig"),
        "mtrl.config.nn": ("MultiHeadConfig", "NeuralNetworkConfig", "VanillaNetworkConfig"),
        "mtrl.config.optim": ("OptimizerConfig", "CAGradConfig"),
        "mtrl.config.rl": ("OffPolicyTrainingConfig",),
        "mtrl.envs": ("MetaworldConfig",),
        "mtrl.experiment": ("Experiment",),
        "mtrl.rl.algorithms": ("MTSACConfig",),
    }
    for mod, attrs in names.items():
        m = importlib.import_module(mod)
        for a in attrs:
            assert hasattr(m, a), (mod, a)


def test_initialize_refuses_unsupported_cagrad_combinations():
    """Raised before any engine is created (no device call)."""
    from fake_env import FakeMetaworldConfig
    from mtrl.config.optim import CAGradConfig, OptimizerConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    env = FakeMetaworldConfig(env_id="MT10")
    T = 10
    plain = OptimizerConfig(max_grad_norm=1.0)
    ca = CAGradConfig(num_tasks=T, max_grad_norm=1.0, cagrad_optimizer=plain)
    with pytest.raises(NotImplementedError, match="CAGrad on one network only"):
        MTSAC.initialize(_algo(ca, plain, T), env, seed=1)
    with pytest.raises(NotImplementedError, match="CAGrad on one network only"):
        MTSAC.initialize(_algo(plain, ca, T), env, seed=1)
    with pytest.raises(ValueError, match="num_tasks must equal"):
        MTSAC.initialize(_algo(ca, CAGradConfig(num_tasks=T + 1, cagrad_optimizer=plain), T), env, seed=1)
    with pytest.raises(NotImplementedError, match="use_task_weights"):
        MTSAC.initialize(_algo(ca, ca, T, use_task_weights=True), env, seed=1)
    with pytest.raises(NotImplementedError, match="sharded"):
        MTSAC.initialize(_algo(ca, ca, T), env, seed=1, task_shard=(0, 5))
