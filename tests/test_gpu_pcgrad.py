"""PCGrad gradient surgery on the GPU (mtrl/optim/pcgrad.py, PCGradConfig on both optimizers).

* the kernels alone (pcgrad.hip) on a matrix loaded with set_task_gradients: Gram against numpy float64,
  the solve against mtrl_amd.pcgrad.pcgrad_from_gram on the device Gram, the combine against the fp32
  ordered sum, read back through the padded gradient buffer;
* three PCGrad steps against the float64 oracle (tests/pcgrad_oracle.py) with pinned task orders and
  injected noise, at fp32, split3 and split2h;
* the device path (update_many, orders drawn on the device), the shared noise of the split losses, the
  mode's contracts, and the compat trainer with PCGradConfig on both networks.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import pcgrad_oracle as po
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5  # tests/test_gpu_update.py


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


# ---------------------------------------------------------------------------- kernels alone
def _test_matrix(T, P):
    """Mixed magnitudes, zero columns, tiny entries: the matrix of test_device_statistics_exact."""
    rng = np.random.default_rng(T)
    G = (rng.standard_normal((T, P)) * rng.choice([1e-4, 1e-2, 1.0, 3.0], size=(T, P))).astype(np.float32)
    G[:, rng.choice(P, P // 7, replace=False)] = 0.0
    G[0, :4] = [np.float32(1e-30), np.float32(-1e-30), 2.0, -2.0]
    return G


@pytest.mark.parametrize("which", [0, 1], ids=["critic", "actor"])
@pytest.mark.parametrize("T", [3, 10, 50])
def test_gram_solve_combine_alone(T, which):
    from mtrl_amd import _lib as L
    from mtrl_amd.pcgrad import pcgrad_from_gram

    # P is never a multiple of the 64-column tile (ragged last tile); the T = 3 critic's is no multiple of 4
    # either (6 head biases: the scalar-load forms), the others are (the 16-byte-load forms)
    W = {3: 32, 10: 64, 50: 32}[T]
    e = _engine(T, W, 2)
    P = e.task_gradient_size(which)
    assert P % 64 != 0 and ((P % 4 != 0) if (T, which) == (3, 0) else (P % 4 == 0))
    G = _test_matrix(T, P)
    e.set_task_gradients(which, G)
    G64 = G.astype(np.float64)
    want = G64 @ G64.T
    gram = e.task_gram(which)
    np.testing.assert_allclose(gram, want, rtol=2e-6, atol=1e-6 * np.abs(want).max())
    np.testing.assert_array_equal(gram, gram.T)
    # solve on the device Gram
    for cosine in (False, True):
        perm = np.random.default_rng(T + 5).permutation(T)
        w, logs = e.task_pcgrad_solve(which, perm, cosine)
        w_ref, logs_ref = pcgrad_from_gram(gram, perm, cosine)
        assert logs_ref["n_grad_conflicts"] > 0
        np.testing.assert_allclose(w, w_ref, rtol=1e-6)
        assert logs["n_grad_conflicts"] == logs_ref["n_grad_conflicts"]
        for k, v in logs_ref.items():
            if np.isnan(v):
                assert not cosine and np.isnan(logs[k]), k
            else:
                assert abs(logs[k] - v) <= 1e-6 * abs(v), (k, logs[k], v)
    # combine: the fp32 ordered sum, through the padded gradient buffer and back
    acc = np.zeros(P, np.float32)
    for t in range(T):
        acc = acc + w[t] * G[t]
    out = e.task_combine(which, w)
    ulp = np.spacing(np.abs(acc))
    assert np.all(np.abs(out.astype(np.float64) - acc.astype(np.float64)) <= 2 * ulp)
    # every leaf in its place: one-hot weights return row t itself, leaf by leaf
    sizes = [int(np.prod(s)) for _, s in (om.critic_leaf_shapes if which == 0 else om.actor_leaf_shapes)(
        om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W))]
    assert sum(sizes) == P
    t = T - 1
    row = e.task_combine(which, np.eye(T, dtype=np.float32)[t])
    o = 0
    for sz in sizes:
        np.testing.assert_array_equal(row[o:o + sz], G[t, o:o + sz])
        o += sz
    # the parameters are untouched by the kernel entries
    assert np.all(np.isfinite(e.get_params(L.CRITIC if which == 0 else L.ACTOR)))
    e.close()


# ---------------------------------------------------------------------------- the step against the oracle
# seeds picked on the CPU (the oracle alone) so that every projection decision of the three steps has
# |cos(g_i^pc, g_j)| >= 1e-3: (3, 32, 4) and (5, 64, 8) hold at seed 23 (2.9e-3 / 3.2e-3), (10, 128, 16) at
# seed 32 (1.26e-3; seed 21 gives 1.2e-4 there)
STEP_CASES = {"t3": (3, 32, 4, 23), "t5": (5, 64, 8, 23), "t10": (10, 128, 16, 32)}


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """Three oracle steps, computed once per shape and shared by the precisions (never mutated)."""
    T, W, n, seed = STEP_CASES[name]
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, seed, head_bound=1.0)
    st0 = st.copy()
    B = n * T
    rng = np.random.default_rng(seed + 7)
    steps = []
    for step in range(3):
        batch = synthetic_batch(T, B, seed=seed + 100 + step, dtype=np.float32)
        # one (n, A) draw shared by the tasks: rows i*T + t see draw i (the reference's vmap key)
        en = np.repeat(rng.standard_normal((n, 4)), T, axis=0).astype(np.float32)
        ec = np.repeat(rng.standard_normal((n, 4)), T, axis=0).astype(np.float32)
        pc, pa = rng.permutation(T), rng.permutation(T)
        st, logs, margins = po.update(cfg, st, batch, en.astype(np.float64), ec.astype(np.float64), pc, pa)
        steps.append((batch, en, ec, pc, pa, logs, margins))
    return cfg, st0, st, steps


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_pcgrad_step_matches_oracle(name, precision):
    from mtrl_amd import _lib as L

    T, W, n, _ = STEP_CASES[name]
    cfg, st0, st, steps = _oracle_run(name)
    # the decisions must not hinge on rounding (100x the 1e-5 per-element gradient tolerance), and the
    # projections must be exercised
    assert min(min(s[6]) for s in steps) >= 1e-3, [s[6] for s in steps]
    assert any(s[5]["metrics/critic_n_grad_conflicts"] > 0 or s[5]["metrics/actor_n_grad_conflicts"] > 0
               for s in steps)
    eng = _engine(T, W, n, precision, capacity=256, actor_max_grad_norm=cfg.actor_max_grad_norm,
                  critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_pcgrad(True)
    _load_state(eng, st0)
    for step, (batch, en, ec, pc, pa, want, _) in enumerate(steps):
        eng.pcgrad_set_order(pc, pa)
        eng.update(batch, en, ec)
        got = eng.logs()
        got_pc = eng.pcgrad_logs()
        oc_, oa_ = eng.pcgrad_get_order()
        np.testing.assert_array_equal(oc_, pc)
        np.testing.assert_array_equal(oa_, pa)
        print(name, precision, step, {k: (got[k], want[k]) for k in got}, {k: (got_pc[k], want[k]) for k in got_pc})
        for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values",
                  "metrics/explore_loss"):
            if k == "losses/alpha_loss" and step == 0:
                assert abs(got[k]) < 1e-6  # log_alpha = 0 at init
                continue
            scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
            assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (name, step, k, got[k], want[k])
        for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
                  "metrics/actor_params_norm", "alpha"):
            assert abs(got[k] - want[k]) < 1e-4 * abs(want[k]), (name, step, k, got[k], want[k])
        for net in ("critic", "actor"):
            assert got_pc[f"metrics/{net}_n_grad_conflicts"] == want[f"metrics/{net}_n_grad_conflicts"]
            for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery"):
                g, w_ = got_pc[f"metrics/{net}_{k}"], want[f"metrics/{net}_{k}"]
                assert abs(g - w_) <= 1e-4 * abs(w_), (name, step, net, k, g, w_)
            assert np.isnan(got_pc[f"metrics/{net}_avg_cosine_similarity"])
            assert np.isnan(got_pc[f"metrics/{net}_avg_cosine_similarity_diff"])
    for which, ref in ((L.ACTOR, st.actor), (L.CRITIC, st.critic), (L.CRITIC_TARGET, st.critic_target),
                       (L.LOG_ALPHA, st.log_alpha)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (which, np.median(d))
        assert d.max() < 2 * 3e-4 * 3 + 1e-6, (which, d.max())
    for which, ref in ((L.ACTOR_ADAM_MU, st.actor_opt.mu), (L.CRITIC_ADAM_MU, st.critic_opt.mu),
                       (L.ACTOR_ADAM_NU, st.actor_opt.nu), (L.CRITIC_ADAM_NU, st.critic_opt.nu)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (which, np.median(d))
        assert d.max() < 2 * 3e-4 * 3 + 1e-6, (which, d.max())
    assert [eng.get_adam_count(i) for i in range(3)] == [3, 3, 3]
    eng.close()


def test_pcgrad_step_cosine_logs_match_oracle():
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, steps = _oracle_run("t5")
    batch, en, ec, pc, pa, _, _ = steps[0]
    _, want, _ = po.update(cfg, st0, batch, en.astype(np.float64), ec.astype(np.float64), pc, pa, cosine_sim_logs=True)
    eng = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_pcgrad(True, cosine_sim_logs=True)
    _load_state(eng, st0)
    eng.pcgrad_set_order(pc, pa)
    eng.update(batch, en, ec)
    got = eng.pcgrad_logs()
    for k, g in got.items():
        assert abs(g - want[k]) <= 1e-4 * abs(want[k]), (k, g, want[k])
    eng.close()


def test_pcgrad_step_mt50():
    """T = 50 (both row halves of the Gram tiles): one step with pinned orders.  With 2450 projection
    decisions per network some have no margin, so only what no decision touches is compared: the losses
    (the actor's sees the critic's update only through Adam's first step, sign(g) lr) and the pre-surgery
    norms."""
    T, W, n, seed = 50, 32, 2, 23
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st0 = po.head_init_state(cfg, seed, head_bound=1.0)
    rng = np.random.default_rng(seed + 7)
    batch = synthetic_batch(T, n * T, seed=seed + 100, dtype=np.float32)
    en = np.repeat(rng.standard_normal((n, 4)), T, axis=0).astype(np.float32)
    ec = np.repeat(rng.standard_normal((n, 4)), T, axis=0).astype(np.float32)
    pc, pa = rng.permutation(T), rng.permutation(T)
    _, want, _ = po.update(cfg, st0, batch, en.astype(np.float64), ec.astype(np.float64), pc, pa)
    eng = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
    eng.set_pcgrad(True)
    _load_state(eng, st0)
    eng.pcgrad_set_order(pc, pa)
    eng.update(batch, en, ec)
    got, got_pc = eng.logs(), eng.pcgrad_logs()
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/qf_values", "metrics/explore_loss"):
        assert abs(got[k] - want[k]) <= LOSS_RTOL * abs(want[k]), (k, got[k], want[k])
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude"):
        assert abs(got[k] - want[k]) < 1e-4 * abs(want[k]), (k, got[k], want[k])
    for net in ("critic", "actor"):
        k = f"metrics/{net}_avg_grad_magnitude_before_surgery"
        assert abs(got_pc[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got_pc[k], want[k])
        k = f"metrics/{net}_n_grad_conflicts"
        assert want[k] > 0 and got_pc[k] > 0 and got_pc[k] * 2 == int(got_pc[k] * 2)
        assert np.isfinite(got_pc[f"metrics/{net}_avg_grad_magnitude"])
    eng.close()


# ---------------------------------------------------------------------------- device path
def test_update_many_draws_orders_on_device():
    T, W, n, seed = STEP_CASES["t5"]
    cfg, st0, _, _ = _oracle_run("t5")

    def make():
        e = _engine(T, W, n, 1, actor_max_grad_norm=cfg.actor_max_grad_norm, critic_max_grad_norm=cfg.critic_max_grad_norm)
        e.set_pcgrad(True)
        _load_state(e, st0)
        e.buffer_fill_synthetic(7)
        e.seed_rng(1)
        return e

    a, b = make(), make()
    orders, logs_a = [], []
    for _ in range(2):
        a.update_many(1)
        orders.append(a.pcgrad_get_order())
        logs_a.append((a.logs(), a.pcgrad_logs()))
    for oc_, oa_ in orders:
        for p in (oc_, oa_):
            np.testing.assert_array_equal(np.sort(p), np.arange(T))
    flat = [tuple(p) for o in orders for p in o]
    assert len(set(flat)) > 1, flat  # the draws differ between networks or steps
    assert all(np.isfinite(v) for lg in logs_a for d in lg for k, v in d.items() if "cosine" not in k)
    # the same two steps in one call: same orders, same logs (no host round trip changes the stream)
    c = make()
    c.update_many(2)
    np.testing.assert_array_equal(c.pcgrad_get_order()[0], orders[1][0])
    np.testing.assert_array_equal(c.pcgrad_get_order()[1], orders[1][1])
    np.testing.assert_equal(c.logs(), logs_a[1][0])
    np.testing.assert_equal(c.pcgrad_logs(), logs_a[1][1])
    # replay: engine b draws the same batch (mtsac_sample advances the same index stream); with the orders
    # a drew and injected noise (the oracle takes eps as an argument; the device stream has its own host model,
    # tests/philox_ref.py, checked in test_gpu_noise_stream.py) its step matches the oracle, and the
    # noise-free log of a's own first step (qf_values = mean Q(s, a_data)) matches the oracle on that batch
    _, batch = b.sample()
    en = np.repeat(np.random.default_rng(3).standard_normal((n, 4)), T, axis=0).astype(np.float32)
    ec = np.repeat(np.random.default_rng(4).standard_normal((n, 4)), T, axis=0).astype(np.float32)
    pc, pa = orders[0]
    _, want, _ = po.update(cfg, st0, batch, en.astype(np.float64), ec.astype(np.float64), pc, pa)
    b.pcgrad_set_order(pc, pa)
    b.update(batch, en, ec)
    got, got_pc = b.logs(), b.pcgrad_logs()
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/qf_values", "metrics/explore_loss"):
        assert abs(got[k] - want[k]) <= LOSS_RTOL * abs(want[k]), (k, got[k], want[k])
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude"):
        assert abs(got[k] - want[k]) < 1e-4 * abs(want[k]), (k, got[k], want[k])
    for net in ("critic", "actor"):
        k = f"metrics/{net}_avg_grad_magnitude_before_surgery"
        assert abs(got_pc[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got_pc[k], want[k])
    k = "losses/qf_values"
    assert abs(logs_a[0][0][k] - want[k]) <= LOSS_RTOL * abs(want[k]), (logs_a[0][0][k], want[k])
    # back to device draws after a pin
    b.pcgrad_set_order(None, None)
    b.update_many(1)
    np.testing.assert_array_equal(np.sort(b.pcgrad_get_order()[0]), np.arange(T))
    for e in (a, b, c):
        e.close()


def test_device_noise_is_shared_by_the_tasks():
    """vmap hands every task the same key: with task-symmetric parameters and identical rows for every
    task, the per-task actor gradients agree on the trunk (they would not with per-row noise)."""
    from mtrl_amd import _lib as L

    T, W, n = 4, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, 5, head_bound=1.0)
    ash, csh = om.actor_leaf_shapes(cfg), om.critic_leaf_shapes(cfg)
    pa, pc = om.unflatten(st.actor, ash), om.unflatten(st.critic, csh)
    pa["head_W"][:], pa["head_b"][:] = pa["head_W"][0], pa["head_b"][0]
    pc["head_W"][:], pc["head_b"][:] = pc["head_W"][:, :1], pc["head_b"][:, :1]
    pa["W0"][39:39 + T] = 0.0
    pc["W0"][:, 4 + 39:4 + 39 + T] = 0.0  # critic input = (action | obs)
    st.actor, st.critic = om.flatten(pa, ash), om.flatten(pc, csh)
    st.critic_target = st.critic.copy()
    rng = np.random.default_rng(9)
    B = n * T
    feat, nfeat = np.repeat(rng.standard_normal((n, 39)), T, axis=0), np.repeat(rng.standard_normal((n, 39)), T, axis=0)
    onehot = np.tile(np.eye(T), (n, 1))
    batch = tuple(x.astype(np.float32) for x in (
        np.concatenate([feat, onehot], axis=1), np.repeat(rng.uniform(-1, 1, (n, 4)), T, axis=0),
        np.concatenate([nfeat, onehot], axis=1), np.zeros((B, 1)), np.repeat(rng.uniform(0, 10, (n, 1)), T, axis=0)))
    eng = _engine(T, W, n, 0)
    eng.set_pcgrad(True)
    _load_state(eng, st)
    eng.update(batch)  # device noise
    G = eng.get_task_gradients(1).astype(np.float64)
    sizes = [int(np.prod(s)) for _, s in ash]
    names = [k for k, _ in ash]
    o, checked = 0, 0
    for k, sz in zip(names, sizes):
        if not k.startswith("head"):
            blk = G[:, o:o + sz]
            if k == "W0":  # the one-hot rows belong to one task each
                blk = blk.reshape(T, 39 + T, W)[:, :39].reshape(T, -1)
            scale = np.abs(blk).max()
            assert scale > 0
            assert np.abs(blk - blk[0]).max() <= 1e-6 * scale, (k, np.abs(blk - blk[0]).max(), scale)
            checked += 1
        o += sz
    assert checked == 2 * cfg.actor_depth
    eng.close()


# ---------------------------------------------------------------------------- contracts
def test_contracts():
    from mtrl_amd._lib import MTSACError
    from mtrl_amd.engine import MTSACEngine, make_config

    sh = MTSACEngine(make_config(num_tasks=4, task_begin=2, task_count=2, obs_dim=43, actor_width=32, critic_width=32,
                                 batch_per_task=4, capacity=64, precision=1))
    with pytest.raises(MTSACError, match="-95"):
        sh.set_pcgrad(True)
    sh.close()
    tw = _engine(3, 32, 4, use_task_weights=1)
    with pytest.raises(MTSACError, match="-95"):
        tw.set_pcgrad(True)
    tw.close()
    e = _engine(3, 32, 4)
    e.set_pcgrad(True)
    with pytest.raises(MTSACError, match="-95"):
        e.enable_graph(True)
    e.enable_graph(False)
    with pytest.raises(MTSACError, match="-22"):
        e.pcgrad_set_order([0, 1, 1], [0, 1, 2])
    e.set_pcgrad(False)
    e.enable_graph(True)
    e.close()


@pytest.mark.parametrize("precision", [0, 1, 3], ids=["fp32", "split3", "split2h"])
def test_plain_step_untouched_when_off(precision):
    """An engine that had PCGrad on and off again steps bit for bit like one that never heard of it."""
    from mtrl_amd import _lib as L

    T, W, n = 3, 32, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W)
    st = po.head_init_state(cfg, 3, head_bound=1e-3)
    outs = []
    for touch in (False, True):
        e = _engine(T, W, n, precision)
        if touch:
            e.set_pcgrad(True, True)
            e.set_pcgrad(False)
        _load_state(e, st)
        for step in range(2):
            batch = synthetic_batch(T, n * T, seed=50 + step, dtype=np.float32)
            en, ec = synthetic_eps(n * T, seed=60 + step, dtype=np.float32)
            e.update(batch, en, ec)
        e.buffer_fill_synthetic(5)
        e.seed_rng(2)
        e.update_many(2)
        outs.append((e.logs(), [e.get_params(w) for w in range(10)]))
        e.close()
    assert outs[0][0] == outs[1][0]
    for x, y in zip(outs[0][1], outs[1][1]):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------- trainer
def test_trainer_with_pcgrad_on_both_networks(tmp_path):
    from fake_env import FakeMetaworldConfig, FakeMTVecEnv
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import PCGradConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.rl.algorithms import MTSACConfig
    from mtrl.rl.algorithms.mtsac import MTSAC
    from mtrl_amd.compat.experiment import NpzCheckpointManager

    T = 10
    opt = PCGradConfig(num_tasks=T, max_grad_norm=1.0)
    algo = MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=opt)),
        critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(num_tasks=T, width=32, optimizer=opt)),
        num_critics=2)
    env_cfg = FakeMetaworldConfig(env_id="MT10")
    tc = OffPolicyTrainingConfig(total_steps=1000, buffer_size=50 * T, batch_size=8 * T, warmstart_steps=5,
                                 evaluation_frequency=10)

    def make(seed):
        agent = MTSAC.initialize(algo, env_cfg, seed=seed, precision="split3")
        return agent, agent.spawn_replay_buffer(env_cfg, tc, 1)

    agent, buf = make(1)
    assert agent.pcgrad
    env = FakeMTVecEnv(T)
    obs, _ = env.reset()
    for _ in range(12):
        nobs, r, term, trunc, _ = env.step(env.action_space.sample())
        buf.add(obs, nobs, env.action_space.sample(), r, np.logical_or(term, trunc))
        obs = nobs
    keys = None
    for _ in range(3):
        agent, logs = agent.update_from_buffer(buf, tc.batch_size, want_logs=True)
        d = dict(logs)
        assert len(logs) == len(d) == 20
        keys = set(d)
        for k, v in d.items():
            if "cosine" in k:
                assert np.isnan(v), (k, v)
            else:
                assert np.isfinite(v), (k, v)
    assert {f"metrics/{net}_{k}" for net in ("critic", "actor") for k in po.PC_KEYS} <= keys
    assert agent.engine.get_adam_count(0) == 3 and agent.engine.get_adam_count(1) == 3
    # checkpoint round trip: a fresh agent restored from it takes the same next step (device orders included)
    m = NpzCheckpointManager(tmp_path / "ck")
    buf.persist_rng_state = True  # keep the index stream's position too (off by default, as the reference)
    m.save(3, agent, buffer=buf, metadata={"step": 3})
    a2, buf2 = make(11)
    meta, bck = m.restore(m.latest_step(), a2, buf2)
    buf2.load_checkpoint(bck)
    assert meta == {"step": 3}
    agent, l1 = agent.update_from_buffer(buf, tc.batch_size, want_logs=True)
    a2, l2 = a2.update_from_buffer(buf2, tc.batch_size, want_logs=True)
    d1, d2 = dict(l1), dict(l2)
    for k in d1:
        assert d1[k] == d2[k] or (np.isnan(d1[k]) and np.isnan(d2[k])), (k, d1[k], d2[k])
    for w in range(10):
        np.testing.assert_array_equal(agent.engine.get_params(w), a2.engine.get_params(w))
    np.testing.assert_array_equal(agent.engine.pcgrad_get_order()[0], a2.engine.pcgrad_get_order()[0])
