"""GradNorm on the GPU (mtrl/optim/gradnorm.py, GradNormConfig on both optimizers).

* the solve kernel alone (gradnorm.hip) on a matrix loaded with set_task_gradients, against
  mtrl_amd.gradnorm.gradnorm_from_gram on the device Gram: the reference form (zero gradient, the inner
  count advancing) and the weighted form (where the inner optimizer does work), then the combine with the
  returned weights;
* the per-task loss values the step reduces on the device against the float64 oracle's;
* three GradNorm steps against the float64 oracle (tests/gradnorm_oracle.py) with injected noise, at fp32,
  split3 and split2h, one step at T = 50, and one weighted-form case;
* the device path (update_many), the mode's contracts, the state through get / set, and the compat
  trainer with GradNormConfig on both networks (logs, checkpoint, rebuild).

The weighted form takes sign decisions (sign(d_t)); a case is compared only where the host statement's
sign_margin is at least 1e-3, far above what fp32 state and task losses can move.  The seeds below were
picked on the CPU, with the host statement alone, so that every weighted case meets it.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import gradnorm_oracle as go
import pcgrad_oracle as po
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om
from test_gpu_cagrad import STEP_CASES, _engine, _load_state, _noise, _test_matrix

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5  # tests/test_gpu_cagrad.py
NORM_RTOL = 1e-4
MARGIN = 1e-3
# the weighted step case starts from unequal weights: from ones, with every row clipped to norm 1 and every
# rate 1 at the first step, all d_t are rounding noise around zero and no sign is decided
WEIGHTED_START = (1.0, 2.0, 0.5, 1.5, 0.75)
ULP1 = float(np.spacing(np.float32(1.0)))
# (T, which) -> seed of the weighted case's state and losses (default 0): see the module docstring
SOLVE_SEEDS = {(33, 0): 2, (50, 1): 1}


# ---------------------------------------------------------------------------- the solve alone
def _weighted_case(T, seed):
    """A state with unequal weights and latched first losses, and two steps' losses with r over 0.5 .. 2."""
    from mtrl_amd.gradnorm import GradNormState, renormalise

    rng = np.random.default_rng(1000 * T + seed)
    st = GradNormState(task_weights=renormalise(rng.uniform(0.5, 2.0, T), T),
                       original_losses=rng.uniform(1.0, 2.0, T).astype(np.float32), count=0,
                       mu=np.zeros(T, np.float32), nu=np.zeros(T, np.float32))
    losses = [(st.original_losses * rng.uniform(0.6, 1.6, T)).astype(np.float32) for _ in range(3)]
    return st, losses


def _check(got_w, got_st, got, want_w, want_st, want, exact_zero_moments):
    np.testing.assert_allclose(got_w, want_w, rtol=1e-6)
    np.testing.assert_allclose(got_st.task_weights, want_st.task_weights, rtol=1e-6)
    np.testing.assert_allclose(got_st.original_losses, want_st.original_losses, rtol=1e-6)
    assert got_st.count == want_st.count
    if exact_zero_moments:
        assert np.all(got_st.mu == 0.0) and np.all(got_st.nu == 0.0)
        assert np.all(want_st.mu == 0.0) and np.all(want_st.nu == 0.0)
    else:
        np.testing.assert_allclose(got_st.mu, want_st.mu, rtol=1e-6)
        np.testing.assert_allclose(got_st.nu, want_st.nu, rtol=1e-6)
    np.testing.assert_array_equal(got["task_weights"], got_st.task_weights)
    np.testing.assert_array_equal(got["original_losses"], got_st.original_losses)
    assert abs(got["grad_magnitude"] - want["grad_magnitude"]) <= 1e-6 * abs(want["grad_magnitude"])
    if np.isnan(want["gradnorm_loss"]):
        assert np.isnan(got["gradnorm_loss"])
    else:
        assert abs(got["gradnorm_loss"] - want["gradnorm_loss"]) <= 1e-6 * abs(want["gradnorm_loss"])


@pytest.mark.parametrize("which", [0, 1], ids=["critic", "actor"])
@pytest.mark.parametrize("T", [2, 3, 10, 33, 50, 64])
def test_solve_alone(T, which):
    from mtrl_amd.gradnorm import gradnorm_from_gram, gradnorm_init

    W = 64 if T == 10 else 32
    e = _engine(T, W, 2)
    P = e.task_gradient_size(which)
    G = _test_matrix(T, P)
    nrm = np.linalg.norm(G.astype(np.float64), axis=1)
    assert (nrm > 1.0).any() and (nrm < 1.0).any()
    e.set_task_gradients(which, G)
    gram = e.task_gram(which)
    rng = np.random.default_rng(T)
    # the reference form, three threaded calls: the latch (one task's first loss is inf), losses of both
    # signs (gradnorm_loss NaN, and only it), the weights where they started, the count advancing
    for iw in (None, 0.5 + np.arange(T) % 4):
        st_d = st_h = gradnorm_init(T, iw)
        w_start = st_h.task_weights.copy()
        for call in range(3):
            L = rng.uniform(1.0, 2.0, T).astype(np.float32)
            if call == 0:
                L[T // 2] = np.inf
            if call == 2:
                L[0] = -L[0]  # a negative rate
            w, st_d, logs = e.task_gradnorm_solve(which, L, st_d)
            w_ref, st_h, ref = gradnorm_from_gram(gram, L, st_h)
            _check(w, st_d, logs, w_ref, st_h, ref, exact_zero_moments=True)
            assert st_d.count == call + 1
            assert np.abs(st_d.task_weights.astype(np.float64) - w_start).max() <= ULP1 * w_start.max()
            assert np.isposinf(st_d.original_losses[T // 2]) == (call == 0)
        assert np.isnan(ref["gradnorm_loss"])
    # the weighted form, two consecutive calls from unequal weights: the inner Adam at work
    st_h, losses = _weighted_case(T, SOLVE_SEEDS.get((T, which), 0))
    st_d, w0 = st_h, st_h.task_weights.copy()
    for call in range(2):
        w, st_d, logs = e.task_gradnorm_solve(which, losses[call], st_d, weighted_norms=True)
        w_ref, st_h, ref = gradnorm_from_gram(gram, losses[call], st_h, weighted_norms=True)
        assert np.all(ref["rates"] > 0.4) and np.all(ref["rates"] < 2.5)
        assert ref["sign_margin"] >= MARGIN, (T, which, call, ref["sign_margin"])  # a condition: change the seed
        print(T, which, call, "margin", ref["sign_margin"], logs["sign_margin"])
        _check(w, st_d, logs, w_ref, st_h, ref, exact_zero_moments=False)
        assert abs(logs["sign_margin"] - ref["sign_margin"]) <= 1e-4 * ref["sign_margin"]
    assert st_d.count == 2 and np.abs(st_d.task_weights - w0).max() > 1e-4
    # per_task_clip off, another asymmetry, inner lr, eps and clip (and none) reach the kernel
    for kw in (dict(per_task_clip=False), dict(asymmetry=0.5, inner_lr=1e-2, inner_eps=1e-3, inner_max_grad_norm=0.05),
               dict(per_task_clip=False, inner_max_grad_norm=None, inner_lr=5e-3)):
        s0, _ = _weighted_case(T, SOLVE_SEEDS.get((T, which), 0))
        w2, st2, logs2 = e.task_gradnorm_solve(which, losses[2], s0, weighted_norms=True, **kw)
        w2_ref, st2_ref, ref2 = gradnorm_from_gram(gram, losses[2], s0, weighted_norms=True, **kw)
        assert ref2["sign_margin"] >= MARGIN, (T, which, kw, ref2["sign_margin"])
        _check(w2, st2, logs2, w2_ref, st2_ref, ref2, exact_zero_moments=False)
        assert np.abs(w2 - w).max() > 1e-5  # not the defaults' answer
    w_off, _, _ = e.task_gradnorm_solve(which, losses[2], gradnorm_init(T), per_task_clip=False)
    np.testing.assert_array_equal(w_off, np.ones(T, np.float32))  # unclipped rows, weights exactly 1 at these T
    # combine with the returned weights: the fp32 ordered sum, through the padded gradient buffer and back
    acc = np.zeros(P, np.float32)
    for t in range(T):
        acc = acc + w[t] * G[t]
    out = e.task_combine(which, w)
    ulp = np.spacing(np.abs(acc))
    assert np.all(np.abs(out.astype(np.float64) - acc.astype(np.float64)) <= 2 * ulp)
    e.close()


# ---------------------------------------------------------------------------- the step against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_run(T, W, n, seed, nsteps, weighted=False):
    """Oracle steps, computed once per shape and shared by the precisions (never mutated)."""
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, seed, head_bound=1.0)
    st0 = st.copy()
    rng = np.random.default_rng(seed + 7)
    gn = go.init(T, WEIGHTED_START if weighted else None)
    steps = []
    for step in range(nsteps):
        batch = synthetic_batch(T, n * T, seed=seed + 100 + step, dtype=np.float32)
        en, ec = _noise(rng, n, T), _noise(rng, n, T)
        st, gn, logs = go.update(cfg, st, gn, batch, en.astype(np.float64), ec.astype(np.float64),
                                 weighted_norms=weighted, require_margin=MARGIN if weighted else None)
        steps.append((batch, en, ec, logs, gn))
    return cfg, st0, st, steps


def _run_and_compare(T, W, n, seed, nsteps, precision, weighted=False):
    from mtrl_amd import _lib as L

    cfg, st0, st, steps = _oracle_run(T, W, n, seed, nsteps, weighted)
    eng = _engine(T, W, n, precision, capacity=256, actor_max_grad_norm=cfg.actor_max_grad_norm,
                  critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_gradnorm(True, weighted_norms=weighted, initial_weights=WEIGHTED_START if weighted else None)
    _load_state(eng, st0)
    first = None
    for step, (batch, en, ec, want, gn) in enumerate(steps):
        eng.update(batch, en, ec)
        got, got_gn = eng.logs(), eng.gradnorm_logs()
        print(T, precision, step, {k: (got[k], want[k]) for k in got},
              {k: (got_gn[k], want[k]) for k in got_gn if "gradnorm_loss" in k})
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
        if step == 0:
            first = {net: want[f"{net}_task_losses"] for net in ("critic", "actor")}
        for w, net in enumerate(("critic", "actor")):
            tw, l0 = got_gn[f"metrics/{net}_task_weights"], got_gn[f"metrics/{net}_original_losses"]
            assert tw.dtype == np.float32 and tw.shape == (T,) and l0.shape == (T,)
            np.testing.assert_allclose(l0, first[net], rtol=LOSS_RTOL)
            np.testing.assert_allclose(want[f"metrics/{net}_original_losses"], first[net], rtol=1e-6)
            dev = eng.gradnorm_state(w)
            assert dev.count == step + 1 == gn[w].count
            if weighted:
                np.testing.assert_allclose(tw, want[f"metrics/{net}_task_weights"], rtol=1e-5)
                np.testing.assert_allclose(dev.mu, gn[w].mu, rtol=1e-3, atol=1e-6 * np.abs(gn[w].mu).max())
                g, w_ = got_gn[f"metrics/{net}_gradnorm_loss"], want[f"metrics/{net}_gradnorm_loss"]
                assert abs(g - w_) <= NORM_RTOL * abs(w_), (step, net, g, w_)
            else:
                assert np.abs(tw.astype(np.float64) - 1.0).max() <= ULP1
                assert np.abs(want[f"metrics/{net}_task_weights"].astype(np.float64) - 1.0).max() <= ULP1
                assert np.all(dev.mu == 0.0) and np.all(dev.nu == 0.0)
    if weighted:
        tw = eng.gradnorm_state(0).task_weights
        assert np.abs(tw - go.init(T, WEIGHTED_START)[0].task_weights).max() > 1e-4
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
def test_gradnorm_step_matches_oracle(name, precision):
    _run_and_compare(*STEP_CASES[name], 3, precision)


def test_gradnorm_step_mt50():
    _run_and_compare(50, 32, 2, 23, 1, 1)


def test_gradnorm_step_weighted_form():
    """The oracle asserts r > 0 and sign_margin >= 1e-3 at every solve of this case (checked on the CPU
    when the case was chosen)."""
    _run_and_compare(*STEP_CASES["t5"], 3, 1, weighted=True)


def test_task_losses_match_oracle():
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, steps = _oracle_run(T, W, n, seed, 3)
    batch, en, ec, want, _ = steps[0]
    eng = _engine(T, W, n, 1, capacity=256, actor_max_grad_norm=cfg.actor_max_grad_norm,
                  critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_gradnorm(True)
    _load_state(eng, st0)
    eng.update(batch, en, ec)
    got, logs = eng.gradnorm_task_losses(), eng.logs()
    print(got, want["critic_task_losses"], want["actor_task_losses"])
    np.testing.assert_allclose(got[0], want["critic_task_losses"], rtol=1e-5)
    np.testing.assert_allclose(got[1], want["actor_task_losses"], rtol=1e-5)
    assert abs(got[0].astype(np.float64).mean() - logs["losses/qf_loss"]) <= 1e-6 * abs(logs["losses/qf_loss"])
    assert abs(got[1].astype(np.float64).mean() - logs["losses/actor_loss"]) <= 1e-6 * abs(logs["losses/actor_loss"])
    eng.close()


# ---------------------------------------------------------------------------- device path
def _gn_snapshot(e):
    out = []
    for w in range(2):
        s = e.gradnorm_state(w)
        out += [s.task_weights, s.original_losses, s.mu, s.nu, np.array([s.count])]
    return out


def _snapshot(e):
    return e.logs(), e.gradnorm_logs(), [e.get_params(w) for w in range(10)] + _gn_snapshot(e)


def _assert_same(x, y):
    assert x[0] == y[0]
    np.testing.assert_equal(x[1], y[1])
    for a, b in zip(x[2], y[2]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("weighted", [False, True], ids=["reference", "weighted"])
def test_update_many_equals_single_device_batch_updates(weighted):
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, _ = _oracle_run(T, W, n, seed, 3)

    def make():
        e = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
        e.set_gradnorm(True, weighted_norms=weighted, initial_weights=[1.0, 2.0, 0.5, 1.5, 1.0])
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
    assert a.gradnorm_state(0).count == a.gradnorm_state(1).count == 3
    a.close()
    b.close()


# ---------------------------------------------------------------------------- contracts
def test_contracts():
    from mtrl_amd._lib import MTSACError
    from mtrl_amd.engine import MTSACEngine, make_config

    sh = MTSACEngine(make_config(num_tasks=4, task_begin=2, task_count=2, obs_dim=43, actor_width=32, critic_width=32,
                                 batch_per_task=4, capacity=64, precision=1))
    with pytest.raises(MTSACError, match="-95"):
        sh.set_gradnorm(True)
    sh.close()
    tw = _engine(3, 32, 4, use_task_weights=1)
    with pytest.raises(MTSACError, match="-95"):
        tw.set_gradnorm(True)
    tw.close()
    e = _engine(3, 32, 4)
    with pytest.raises(MTSACError, match="-22"):
        e.gradnorm_state(0)  # never set up
    for bad in (dict(asymmetry=float("nan")), dict(inner_lr=float("inf")), dict(inner_eps=(1e-5, float("nan"))),
                dict(inner_max_grad_norm=float("inf")), dict(initial_weights=[1.0, -1.0, 0.0]),
                dict(initial_weights=[1.0, float("nan"), 1.0])):
        with pytest.raises(MTSACError, match="-22"):
            e.set_gradnorm(True, **bad)
    e.enable_graph(True)  # nothing above switched the mode on
    e.set_gradnorm(True)
    with pytest.raises(MTSACError, match="-95"):
        e.enable_graph(True)
    e.enable_graph(False)
    with pytest.raises(MTSACError, match="-16"):
        e.set_pcgrad(True)
    with pytest.raises(MTSACError, match="-16"):
        e.set_cagrad(True)
    e.set_gradnorm(False)
    e.enable_graph(True)
    e.set_pcgrad(True)
    with pytest.raises(MTSACError, match="-16"):
        e.set_gradnorm(True)
    e.set_pcgrad(False)
    e.set_cagrad(True)
    with pytest.raises(MTSACError, match="-16"):
        e.set_gradnorm(True)
    e.set_cagrad(False)
    # on again: a fresh state
    e.set_gradnorm(True, initial_weights=[1.0, 2.0, 3.0])
    s = e.gradnorm_state(1)
    np.testing.assert_array_equal(s.task_weights, np.array([0.5, 1.0, 1.5], np.float32))
    assert np.all(np.isposinf(s.original_losses)) and s.count == 0 and not s.mu.any() and not s.nu.any()
    e.set_gradnorm(False)
    e.set_gradnorm(True)
    np.testing.assert_array_equal(e.gradnorm_state(1).task_weights, np.ones(3, np.float32))
    e.set_gradnorm(False)
    e.close()


@pytest.mark.parametrize("mode", ["plain", "pcgrad"])
def test_other_steps_untouched_after_a_toggle(mode):
    """An engine that had GradNorm on and off again takes the plain step, and the PCGrad step, bit for bit
    like one that never heard of it."""
    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, 3, head_bound=1.0 if mode == "pcgrad" else 1e-3)
    outs = []
    for touch in (False, True):
        e = _engine(T, W, n, 1)
        if touch:
            e.set_gradnorm(True, weighted_norms=True)
            e.set_gradnorm(False)
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


def test_state_survives_get_and_set():
    """get_state -> a fresh engine -> set_state: the next step is bitwise the same."""
    T, W, n, seed = STEP_CASES["t3"]
    cfg, st0, _, steps = _oracle_run(T, W, n, seed, 3)

    def make():
        e = _engine(T, W, n, 1, capacity=256, actor_max_grad_norm=cfg.actor_max_grad_norm,
                    critic_max_grad_norm=cfg.critic_max_grad_norm)
        e.set_gradnorm(True, weighted_norms=True)
        return e

    a = make()
    _load_state(a, st0)
    for batch, en, ec, _, _ in steps[:2]:
        a.update(batch, en, ec)
    b = make()
    for w in range(10):
        b.set_params(w, a.get_params(w))
    for i in range(3):
        b.set_adam_count(i, a.get_adam_count(i))
    b.set_noise_state(*a.noise_state())
    for w in range(2):
        s = a.gradnorm_state(w)
        assert s.count == 2 and np.all(np.isfinite(s.original_losses)) and np.abs(s.mu).max() > 0
        b.set_gradnorm_state(w, s)
    batch, en, ec, _, _ = steps[2]
    a.update(batch, en, ec)
    b.update(batch, en, ec)
    _assert_same(_snapshot(a), _snapshot(b))
    a.close()
    b.close()


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


def _samples(T, n, seed):
    from mtrl.types import ReplayBufferSamples

    return ReplayBufferSamples(*synthetic_batch(T, n * T, seed=seed, dtype=np.float32))


def test_trainer_with_gradnorm_on_both_networks():
    from fake_env import FakeMetaworldConfig
    from mtrl.config.optim import GradNormConfig, OptimizerConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    T = 3

    class ThreeTasks(FakeMetaworldConfig):  # MetaworldConfig's spaces with three one-hot task columns
        @property
        def num_tasks(self) -> int:
            return T

    plain = OptimizerConfig(max_grad_norm=1.0)
    opt = GradNormConfig(num_tasks=T, max_grad_norm=1.0, gradnorm_optimizer=plain)
    env_cfg = ThreeTasks(env_id="MT3")
    with pytest.raises(NotImplementedError, match="one network only"):
        MTSAC.initialize(_algo(T, opt, plain), env_cfg, seed=1)
    agent = MTSAC.initialize(_algo(T, opt, opt), env_cfg, seed=1, precision="split3")
    assert agent.gradnorm and not agent.pcgrad and not agent.cagrad
    for step in range(2):
        agent, logs = agent.update(_samples(T, 8, 40 + step))
        d = dict(logs)
        assert len(logs) == len(d) == 14
        for net in ("critic", "actor"):
            tw, l0 = d[f"metrics/{net}_task_weights"], d[f"metrics/{net}_original_losses"]
            assert tw.shape == l0.shape == (T,) and np.all(np.isfinite(l0))
            np.testing.assert_array_equal(tw, np.ones(T, np.float32))
        assert all(np.isfinite(v) for k, v in d.items() if np.ndim(v) == 0)
    first = {w: agent.engine.gradnorm_state(w).original_losses.copy() for w in range(2)}
    # checkpoint: a new agent from the state dict takes the next step bitwise alike
    sd = agent.state_dict()
    for net in ("critic", "actor"):
        assert int(sd[f"{net}/opt_state/0/opt_state/1/0/count"]) == 2 and int(sd[f"{net}/opt_state/1/1/0/count"]) == 2
        np.testing.assert_array_equal(sd[f"{net}/opt_state/0/original_losses"], first[0 if net == "critic" else 1])
    other = MTSAC.initialize(_algo(T, opt, opt), env_cfg, seed=5, precision="split3")
    other, _ = other.update(_samples(T, 8, 77))  # same geometry, another history
    other.load_state_dict(sd)
    nxt = _samples(T, 8, 42)
    agent, _ = agent.update(nxt)
    other, _ = other.update(nxt)
    for w in range(10):
        np.testing.assert_array_equal(agent.engine.get_params(w), other.engine.get_params(w))
    for x, y in zip(_gn_snapshot(agent.engine), _gn_snapshot(other.engine)):
        np.testing.assert_array_equal(x, y)
    # another batch size rebuilds the engine: the latched losses and the inner counts survive
    agent, logs = agent.update(_samples(T, 4, 43))
    for w in range(2):
        s = agent.engine.gradnorm_state(w)
        assert s.count == 4
        np.testing.assert_array_equal(s.original_losses, first[w])
    assert agent.engine.get_adam_count(0) == 4 and agent.engine.get_adam_count(1) == 4
    agent.engine.close()
    other.engine.close()
