"""GradNorm on the CPU: the Gram-form host statement (mtrl_amd/gradnorm.py) against the reference's literal
statement with torch.autograd's gradient, the reference form's zero gradient and constant weights pinned,
the weighted form's analytic gradient, sum versus mean, the per-task clip bound, and the config, trainer
and checkpoint surface (mtrl.config.optim.GradNormConfig, MTSAC.initialize's refusals, the opt_state
layout of the reference's chain)."""

from __future__ import annotations

import numpy as np
import pytest

from cagrad_oracle import matrix_families

FAMILIES = ("random", "half_conflicting", "cancelling", "tiny", "zero")
ULP1 = float(np.spacing(np.float32(1.0)))  # float32 ulp at 1 (2^-23); just below 1 it is half of that


def _losses(rng, T, step):
    """Positive, changing from step to step, ratios to the first within about 0.5 .. 2."""
    return rng.uniform(1.0, 2.0, T) * (1.0 + 0.1 * step)


def _nonuniform(T):
    return 0.5 + np.arange(T) % 4


# ---------------------------------------------------------------------------- 1. Gram form against the literal statement
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a - b).max())


def _run(fn, arg, T, weighted, perm=None):
    """Three threaded steps; the combine weights, task weights and Adam moments of every step (task order
    undone)."""
    from mtrl_amd.gradnorm import gradnorm_init

    rng = np.random.default_rng(11 * T + weighted)
    iw = rng.uniform(0.5, 2.0, T)
    p = np.arange(T) if perm is None else perm
    inv = np.argsort(p)
    st = gradnorm_init(T, iw[p] if weighted else None)
    out = []
    for step in range(3):
        L = _losses(rng, T, step)
        upd, st, logs = fn(arg, L[p], st, weighted_norms=weighted)
        out.append((np.asarray(upd), logs["combine_weights"][inv], st.task_weights[inv], st.mu[inv], st.nu[inv],
                    logs["gradnorm_loss"], logs["grad_magnitude"], logs["sign_margin"]))
    return out


def _worst(got, want, loss_scale):
    """Largest relative difference (each vector against its largest entry) over the combine weights, the
    state and the logs; gradnorm_loss, a sum of differences of norms that cancel when every row is clipped
    to the same norm, against the sum of the norms."""
    worst = 0.0
    for g, w in zip(got, want):
        for k in (1, 2, 3, 4, 6):
            worst = max(worst, _rel(g[k], w[k]))
        worst = max(worst, abs(g[5] - w[5]) / max(loss_scale, 1e-300))
    return worst


@pytest.mark.parametrize("weighted", [False, True], ids=["reference", "weighted"])
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("T", [2, 3, 10, 50])
def test_gram_form_matches_literal_statement(T, kind, weighted):
    """The rule of test_cagrad_cpu.py::test_gram_form_matches_literal_statement: the bound is 10x the
    difference between two runs of the literal statement with the task rows in forward and in reversed
    order (a pure reordering of float64 sums), floor 1e-12.  Compared: the combine weights, the state and
    the logs of three threaded steps; the update itself against the forward error scale of its sum,
    (|w| |M|) elementwise (on cancelling rows the update is rounding noise around zero)."""
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram

    M = matrix_families(T, 200, T)[kind]
    want = _run(gradnorm_direct, M, T, weighted)
    rev = _run(gradnorm_direct, M[::-1], T, weighted, perm=np.arange(T)[::-1])
    scale = np.minimum(np.linalg.norm(M, axis=1), 1.0).sum()
    reorder = _worst(rev, want, scale)
    bound = max(10.0 * reorder, 1e-12)
    got = _run(gradnorm_from_gram, M @ M.T, T, weighted)
    diff = _worst(got, want, scale)
    print(T, kind, weighted, "reorder", reorder, "gram form", diff)
    assert diff <= bound, (diff, bound)
    if weighted and kind != "zero":
        # no sign decision near a flip (the two task orders differ by float32 roundings of the state, 1e-7)
        assert min(w[7] for w in want) >= 1e-5
    for g, w in zip(got, want):
        upd = g[1] @ M  # from_gram hands back the combine weights
        scale = (np.abs(w[1]) @ np.abs(M)).max()
        assert np.abs(upd - w[0]).max() <= bound * scale


# ---------------------------------------------------------------------------- 2. the reference form, pinned
@pytest.mark.parametrize("T,start", [(10, "ones"), (41, "ones"), (50, "ones"), (55, "ones"), (10, "nonuniform"),
                                     (41, "nonuniform")])
def test_reference_form_weights_never_move(T, start):
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram, gradnorm_init

    rng = np.random.default_rng(T)
    iw = None if start == "ones" else _nonuniform(T)
    w0 = gradnorm_init(T, iw).task_weights
    assert w0.dtype == np.float32 and abs(float(w0.sum(dtype=np.float64)) - T) <= T * ULP1
    if start == "ones":  # the one-ulp table of DESIGN.md section 12
        np.testing.assert_array_equal(w0, np.float32(1.0 - 2.0 ** -24 if T in (41, 47, 55, 61) else 1.0))
    sd = sg = gradnorm_init(T, iw)
    for step in range(30):
        M = matrix_families(T, 60, 100 + step)["random"]
        L = rng.standard_normal(T) * (1.0 + step)  # changing, of both signs: gradnorm_loss is NaN at times
        _, sd, ld = gradnorm_direct(M, L, sd)
        _, sg, lg = gradnorm_from_gram(M @ M.T, L, sg)
        assert np.all(ld["weights_grad"] == 0.0) and np.all(lg["weights_grad"] == 0.0)  # autograd's: exactly 0
        for s in (sd, sg):
            assert np.all(s.mu == 0.0) and np.all(s.nu == 0.0)
            assert np.abs(s.task_weights.astype(np.float64) - w0).max() <= ULP1 * np.abs(w0).max()
            assert s.task_weights.dtype == np.float32
    assert sd.count == sg.count == 30
    np.testing.assert_array_equal(sd.task_weights, sg.task_weights)


def test_renormalisation_table():
    """(ones(T) / T) * T in float32, T = 1 .. 64: exactly 1 except at T = 41, 47, 55, 61 (1 - 2^-24)."""
    from mtrl_amd.gradnorm import gradnorm_init

    off = [T for T in range(1, 65) if np.any(gradnorm_init(T).task_weights != np.float32(1.0))]
    assert off == [41, 47, 55, 61]
    for T in off:
        np.testing.assert_array_equal(gradnorm_init(T).task_weights, np.float32(1.0 - 2.0 ** -24))


def test_reference_form_edge_losses():
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram, gradnorm_init

    T = 6
    M = matrix_families(T, 40, 3)["random"]
    L = np.array([1.5, -0.7, 0.0, np.inf, 2.0, -3.0])
    for fn, arg in ((gradnorm_direct, M), (gradnorm_from_gram, M @ M.T)):
        st = gradnorm_init(T)
        for step in range(3):
            out, st, logs = fn(arg, L * (1.0 + step), st)
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(st.task_weights))
            assert np.all(st.mu == 0.0) and np.all(st.nu == 0.0) and st.count == step + 1
            assert np.isnan(logs["gradnorm_loss"])  # the negative rates' NaN stays in the loss, and only there
        np.testing.assert_array_equal(st.task_weights, np.ones(T, np.float32))


def test_latch():
    from mtrl_amd.gradnorm import gradnorm_from_gram, gradnorm_init

    T = 4
    G = (lambda M: M @ M.T)(matrix_families(T, 40, 5)["random"])
    st = gradnorm_init(T)
    assert np.all(np.isposinf(st.original_losses))
    _, st, _ = gradnorm_from_gram(G, np.array([1.0, np.inf, 3.0, 4.0]), st)
    np.testing.assert_array_equal(st.original_losses, np.array([1.0, np.inf, 3.0, 4.0], np.float32))
    _, st, _ = gradnorm_from_gram(G, np.array([9.0, 2.5, 9.0, 9.0]), st)
    np.testing.assert_array_equal(st.original_losses, np.array([1.0, 2.5, 3.0, 4.0], np.float32))
    _, st, logs = gradnorm_from_gram(G, np.array([7.0, 7.0, 7.0, 7.0]), st)
    np.testing.assert_array_equal(st.original_losses, np.array([1.0, 2.5, 3.0, 4.0], np.float32))
    np.testing.assert_array_equal(logs["original_losses"], st.original_losses)


# ---------------------------------------------------------------------------- 3. the weighted form
@pytest.mark.parametrize("T", [3, 7, 50])
def test_weighted_gradient_matches_autograd(T):
    import torch

    from mtrl_amd.gradnorm import weighted_grad

    rng = np.random.default_rng(T)
    checked = 0
    for _ in range(20):
        w = rng.uniform(0.3, 2.0, T) * rng.choice([-1.0, 1.0], T, p=[0.2, 0.8])
        nt = rng.uniform(0.05, 1.0, T)
        r = rng.uniform(0.5, 2.0, T)
        loss, d, avg, g = weighted_grad(w, nt, r, 0.12)
        if np.abs(d).min() / avg < 1e-6:
            continue
        wt = torch.tensor(w, requires_grad=True)
        N = torch.abs(wt) * torch.from_numpy(nt)
        lt = (N - N.mean() * torch.from_numpy(r) ** 0.12).abs().sum()
        (gt,) = torch.autograd.grad(lt, wt)
        assert abs(loss - lt.item()) <= 1e-13 * abs(lt.item())
        assert np.abs(g - gt.numpy()).max() <= 1e-12 * np.abs(gt.numpy()).max()
        checked += 1
    assert checked >= 15


def test_weighted_form_moves_the_weights():
    """The inputs the device tests reuse: checked with the host statement alone."""
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram, gradnorm_init

    T = 10
    M = matrix_families(T, 200, T)["random"]
    rng = np.random.default_rng(1)
    for fn, arg in ((gradnorm_from_gram, M @ M.T), (gradnorm_direct, M)):
        st = gradnorm_init(T)
        w0 = st.task_weights.copy()
        for step in range(5):
            _, st, logs = fn(arg, _losses(rng, T, step), st, weighted_norms=True)
            assert np.all(logs["rates"] > 0) and np.isfinite(logs["gradnorm_loss"])
        w = st.task_weights.astype(np.float64)
        assert np.abs(w - w0).max() > 1e-4 and w.max() / w.min() > 1.0005, (w,)
        assert st.count == 5 and np.abs(st.mu).max() > 0 and np.abs(st.nu).max() > 0
        assert abs(w.sum() - T) <= T * ULP1
    # a negative rate: NaN through jnp.power, into the weights (not guarded)
    L = np.ones(T)
    L[3] = -1.0
    _, st, logs = gradnorm_from_gram(M @ M.T, L * 2.0, gradnorm_from_gram(M @ M.T, np.ones(T), gradnorm_init(T))[1],
                                     weighted_norms=True)
    assert np.isnan(logs["gradnorm_loss"]) and np.all(np.isnan(st.task_weights))


# ---------------------------------------------------------------------------- 4. sum, clip
def test_update_is_a_sum_not_a_mean():
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram, gradnorm_init

    T, P = 8, 30
    row = np.random.default_rng(0).standard_normal(P)
    row *= 0.25 / np.linalg.norm(row)  # below the clip bound
    M = np.tile(row, (T, 1))
    upd, _, logs = gradnorm_direct(M, np.ones(T), gradnorm_init(T))
    assert np.abs(upd - T * row).max() <= 1e-15 * T
    w, _, logs_g = gradnorm_from_gram(M @ M.T, np.ones(T), gradnorm_init(T))
    np.testing.assert_array_equal(w, np.ones(T))
    for lg in (logs, logs_g):  # the logged magnitude stays the mean's
        assert abs(lg["grad_magnitude"] - 0.25) <= 1e-15


def test_per_task_clip_bound_is_one():
    from mtrl.config.optim import GradNormConfig, OptimizerConfig
    from mtrl_amd.compat.rl.algorithms.mtsac import _gradnorm_args
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_from_gram, gradnorm_init

    T, P = 4, 30
    M = np.random.default_rng(2).standard_normal((T, P))
    M *= (np.array([0.3, 0.75, 2.0, 5.0]) / np.linalg.norm(M, axis=1))[:, None]
    inner = OptimizerConfig(max_grad_norm=1.0)
    for mgn, clipped in ((0.5, True), (None, False), (0.0, False), (7.0, True)):
        opt = GradNormConfig(num_tasks=T, gradnorm_optimizer=inner, max_grad_norm=mgn)
        clip = _gradnorm_args(_algo(opt, opt, T))["per_task_clip"]
        assert clip == (clipped, clipped)
        w, _, _ = gradnorm_from_gram(M @ M.T, np.ones(T), gradnorm_init(T), per_task_clip=clip[0])
        upd, _, _ = gradnorm_direct(M, np.ones(T), gradnorm_init(T), per_task_clip=clip[0])
        norms = np.linalg.norm(w[:, None] * M, axis=1)
        want = np.array([0.3, 0.75, 1.0, 1.0]) if clipped else np.array([0.3, 0.75, 2.0, 5.0])  # 1.0, never 0.5
        assert np.abs(norms - want).max() <= 1e-7
        assert np.abs(w @ M - upd).max() <= 1e-14


# ---------------------------------------------------------------------------- 5. config, trainer, checkpoint
def _algo(actor_opt, critic_opt, T=3, **kw):
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import VanillaNetworkConfig
    from mtrl.rl.algorithms import MTSACConfig

    return MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=VanillaNetworkConfig(width=32, optimizer=actor_opt)),
        critic_config=QValueFunctionConfig(network_config=VanillaNetworkConfig(width=32, optimizer=critic_opt)),
        num_critics=2, **kw)


def test_gradnorm_config_surface():
    import dataclasses

    from mtrl.config.optim import GradNormConfig, OptimizerConfig
    from mtrl_amd.compat.config import optim as compat_optim
    from mtrl_amd.engine import GRADNORM_LOG_KEYS
    from mtrl_amd.gradnorm import LOG_KEYS

    assert GradNormConfig is compat_optim.GradNormConfig
    c = GradNormConfig(num_tasks=10, gradnorm_optimizer=OptimizerConfig(max_grad_norm=1.0))
    assert isinstance(c, OptimizerConfig)
    assert c.requires_split_task_losses is True
    assert (c.num_tasks, c.initial_weights, c.asymmetry, c.max_grad_norm, c.lr, c.adam_eps) == (
        10, None, 0.12, None, 3e-4, 1e-5)
    assert {"num_tasks", "gradnorm_optimizer", "initial_weights", "asymmetry", "max_grad_norm"} <= {
        f.name for f in dataclasses.fields(c)}
    with pytest.raises(TypeError):
        GradNormConfig(num_tasks=3)  # gradnorm_optimizer has no default in the reference either
    assert LOG_KEYS == GRADNORM_LOG_KEYS == ("task_weights", "original_losses")


def test_experiment_script_imports_resolve():
    """Every name experiments/misc/mt10_mtmhsac_gradnorm.py imports from mtrl.*."""
    import importlib

    names = {
        "mtrl.config.networks": ("ContinuousActionPolicyConfig", "QValueFunctionConfig"),
        "mtrl.config.nn": ("MultiHeadConfig", "NeuralNetworkConfig", "VanillaNetworkConfig"),
        "mtrl.config.optim": ("OptimizerConfig", "GradNormConfig"),
        "mtrl.config.rl": ("OffPolicyTrainingConfig",),
        "mtrl.envs": ("MetaworldConfig",),
        "mtrl.experiment": ("Experiment",),
        "mtrl.rl.algorithms": ("MTSACConfig",),
    }
    for mod, attrs in names.items():
        m = importlib.import_module(mod)
        for a in attrs:
            assert hasattr(m, a), (mod, a)


def test_initialize_refuses_unsupported_gradnorm_combinations():
    """Raised before any engine is created (no device call)."""
    from fake_env import FakeMetaworldConfig
    from mtrl.config.optim import CAGradConfig, GradNormConfig, OptimizerConfig
    from mtrl.config.utils import Optimizer
    from mtrl.rl.algorithms.mtsac import MTSAC

    env = FakeMetaworldConfig(env_id="MT10")
    T = 10
    plain = OptimizerConfig(max_grad_norm=1.0)
    gn = GradNormConfig(num_tasks=T, max_grad_norm=1.0, gradnorm_optimizer=plain)
    with pytest.raises(NotImplementedError, match="GradNorm on one network only"):
        MTSAC.initialize(_algo(gn, plain, T), env, seed=1)
    with pytest.raises(NotImplementedError, match="GradNorm on one network only"):
        MTSAC.initialize(_algo(plain, gn, T), env, seed=1)
    with pytest.raises(NotImplementedError, match="one network only"):
        MTSAC.initialize(_algo(gn, CAGradConfig(num_tasks=T, cagrad_optimizer=plain), T), env, seed=1)
    with pytest.raises(ValueError, match="num_tasks must equal"):
        MTSAC.initialize(_algo(gn, GradNormConfig(num_tasks=T + 1, gradnorm_optimizer=plain), T), env, seed=1)
    with pytest.raises(NotImplementedError, match="use_task_weights"):
        MTSAC.initialize(_algo(gn, gn, T, use_task_weights=True), env, seed=1)
    with pytest.raises(NotImplementedError, match="sharded"):
        MTSAC.initialize(_algo(gn, gn, T), env, seed=1, task_shard=(0, 5))
    other = [o for o in Optimizer if o is not Optimizer.Adam][0]
    with pytest.raises(NotImplementedError, match="gradnorm_optimizer must be a plain Adam"):
        MTSAC.initialize(_algo(gn, GradNormConfig(num_tasks=T, gradnorm_optimizer=OptimizerConfig(optimizer=other)), T),
                         env, seed=1)
    with pytest.raises(ValueError, match="max_grad_norm = 0.0"):
        MTSAC.initialize(_algo(GradNormConfig(num_tasks=T, gradnorm_optimizer=OptimizerConfig(max_grad_norm=0.0)), gn, T),
                         env, seed=1)
    with pytest.raises(NotImplementedError, match="asymmetry"):
        MTSAC.initialize(_algo(gn, GradNormConfig(num_tasks=T, gradnorm_optimizer=plain, asymmetry=0.5), T), env,
                         seed=1)


def test_checkpoint_tree_round_trip():
    import test_checkpoint_cpu as tc
    from mtrl_amd.compat import checkpoint as C
    from mtrl_amd.gradnorm import GradNormState

    kw = tc.KW
    T = kw["num_tasks"]
    src = tc._FakeEngine(tc._sizes(kw))
    rng = np.random.default_rng(0)
    states = [GradNormState(task_weights=rng.uniform(0.5, 1.5, T).astype(np.float32),
                            original_losses=np.array([1.0, np.inf, 3.0, -2.0], np.float32) * (w + 1), count=17 + w,
                            mu=rng.standard_normal(T).astype(np.float32),
                            nu=rng.uniform(0, 1, T).astype(np.float32)) for w in range(2)]
    clips = (1.0, None)  # the critic's inner optimizer clipped, the actor's not
    plain = C.agent_tree(kw, src.get_params, src.get_adam_count)
    tree = C.agent_tree(kw, src.get_params, src.get_adam_count, gradnorm=(lambda w: states[w], clips))
    for net, w, inner in (("critic", 0, "1/0"), ("actor", 1, "0")):
        np.testing.assert_array_equal(tree[f"{net}/opt_state/0/task_weights"], states[w].task_weights)
        np.testing.assert_array_equal(tree[f"{net}/opt_state/0/original_losses"], states[w].original_losses)
        assert int(tree[f"{net}/opt_state/0/opt_state/{inner}/count"]) == 17 + w
        np.testing.assert_array_equal(tree[f"{net}/opt_state/0/opt_state/{inner}/mu"], states[w].mu)
        np.testing.assert_array_equal(tree[f"{net}/opt_state/0/opt_state/{inner}/nu"], states[w].nu)
        assert f"{net}/opt_state/1/1/0/count" in tree and f"{net}/opt_state/1/0/count" not in tree
    # everything else is the plain tree with the outer Adam one level down
    moved = {k.replace("/opt_state/1/0/", "/opt_state/1/1/0/") if not k.startswith("alpha") else k: v
             for k, v in plain.items()}
    rest = {k: v for k, v in tree.items() if "/opt_state/0/" not in k or k.startswith("alpha")}
    assert set(rest) == set(moved)
    for k in moved:
        np.testing.assert_array_equal(rest[k], moved[k])
    # and back
    dst = tc._FakeEngine(tc._sizes(kw))
    dst.p = {w: np.zeros_like(v) for w, v in dst.p.items()}
    dst.counts = [0, 0, 0]
    got = {}
    C.load_agent_tree(kw, tree, dst.set_params, dst.set_adam_count, gradnorm=(got.__setitem__, clips))
    for w in tc._sizes(kw):
        np.testing.assert_array_equal(dst.p[w], src.p[w])
    assert dst.counts == src.counts
    for w in range(2):
        assert got[w].count == states[w].count
        for f in ("task_weights", "original_losses", "mu", "nu"):
            np.testing.assert_array_equal(getattr(got[w], f), getattr(states[w], f))
    with pytest.raises(KeyError):  # a plain checkpoint does not load into a GradNorm agent
        C.load_agent_tree(kw, plain, dst.set_params, dst.set_adam_count, gradnorm=(got.__setitem__, clips))


def test_plain_mode_tree_is_unchanged():
    import test_checkpoint_cpu as tc
    from mtrl_amd.compat import checkpoint as C

    st = C.agent_state(tc._Algo(tc._FakeEngine(tc._sizes(tc.KW)), tc.KW))
    want = tc._expected_keys(4, 43, 16, 3, 2)
    assert set(st) == set(want)
    assert not any("/opt_state/0/opt_state" in k or "task_weights" in k for k in st)
