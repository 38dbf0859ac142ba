"""tests/shared_head_ref.py (the float64 shared-head MTSAC step) checked on its own, and the host side of the
shared-head network: leaf order, shapes, known-answer counts, the trainer's refusals, the checkpoint paths."""

from __future__ import annotations

import numpy as np
import pytest

import shared_head_ref as sr
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om


def _cfg(T, W=8, **kw):
    return om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, **kw)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("clip_tw", [False, True])
def test_one_task_equals_the_multi_head_oracle(clip_tw):
    """T = 1: one head either way, so the step is oracle.update's after the leaf permutation (only the norm's
    summation order differs): losses and parameters to 1e-12 relative."""
    cfg = _cfg(1, 16, clip=clip_tw, use_task_weights=clip_tw)
    st = sr.initialize(cfg, 3)
    mh = sr.tied_state(cfg, st)
    for k in range(2):
        batch = synthetic_batch(1, 6, seed=1 + k)
        en, ec = synthetic_eps(6, seed=2 + k)
        st, l1, _ = sr.update(cfg, st, batch, en, ec)
        mh, l2 = om.update(cfg, mh, batch, en, ec)
        for key in l1:
            assert abs(l1[key] - l2[key]) <= 1e-12 * abs(l2[key]), (k, key, l1[key], l2[key])
        for a, b, shv, shm in ((st.actor, mh.actor, sr.actor_shapes(cfg), om.actor_leaf_shapes(cfg)),
                               (st.critic, mh.critic, sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg)),
                               (st.critic_target, mh.critic_target, sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg))):
            assert _rel(sr.tie(a, shv, shm, 1), b) < 1e-12
        assert _rel(st.log_alpha, mh.log_alpha) < 1e-12 or np.all(st.log_alpha == mh.log_alpha)


def test_finite_differences_in_the_shared_head():
    """Central differences of the critic loss and the actor loss in the shared head's kernel and bias, float64,
    T = 3 (the step and bar of tests/test_oracle_mtsac.py: h = 1e-6, 1e-5 max(1, |g|))."""
    T, B = 3, 12
    cfg = _cfg(T)
    st = sr.initialize(cfg, seed=1, head_bound=0.5)
    batch = synthetic_batch(T, B, seed=2)
    en, ec = synthetic_eps(B)
    _, _, gc = sr.critic_loss_grad(cfg, st, batch, en)
    _, ga, _ = sr.actor_loss_grad(cfg, st, batch, ec)
    rng = np.random.default_rng(0)
    for net, g, shapes, loss in (
            ("critic", gc, sr.critic_shapes(cfg), lambda s: sr.critic_loss_grad(cfg, s, batch, en)[0]),
            ("actor", ga, sr.actor_shapes(cfg), lambda s: sr.actor_loss_grad(cfg, s, batch, ec)[0])):
        n_head = sum(int(np.prod(s)) for k, s in shapes if k.startswith("head"))
        head = np.arange(g.size - n_head, g.size)  # the head's leaves come last
        assert np.abs(g[head]).max() > 0
        for i in rng.choice(head, 12, replace=False):
            h = 1e-6
            s1, s2 = st.copy(), st.copy()
            getattr(s1, net)[i] += h
            getattr(s2, net)[i] -= h
            fd = (loss(s1) - loss(s2)) / (2 * h)
            assert abs(fd - g[i]) < 1e-5 * max(1.0, abs(g[i])), (net, i, fd, g[i])


def test_leaf_order_shapes_and_known_answer_counts():
    from mtrl_amd.init import init_vanilla, vanilla_leaf_shapes

    # MT10 / W400 / A4: 344,008 actor parameters, 685,602 critic parameters (2 members)
    cfg = om.OracleConfig(num_tasks=10, obs_dim=49)
    assert om.num_params(sr.actor_shapes(cfg)) == sr.param_count(49, 400, 3, 8) == 344_008
    assert om.num_params(sr.critic_shapes(cfg)) == sr.param_count(53, 400, 3, 1, 2) == 685_602
    a, c = init_vanilla(10, 49, 4, 400, 3, 400, 3, 2, seed=1)
    assert a.size == 344_008 and c.size == 685_602 and a.dtype == c.dtype == np.float32
    assert vanilla_leaf_shapes(49, 400, 3, 8, None) == sr.actor_shapes(cfg)
    assert vanilla_leaf_shapes(53, 400, 3, 1, 2) == sr.critic_shapes(cfg)
    names = [k for k, _ in sr.critic_shapes(cfg)]
    assert names == ["b0", "W0", "b1", "W1", "b2", "W2", "head_b", "head_W"]  # layer_0 .. layer_D, bias < kernel
    assert dict(sr.critic_shapes(cfg))["head_W"] == (2, 400, 1) and dict(sr.actor_shapes(cfg))["head_W"] == (400, 8)
    # init: he_uniform trunk, zero biases, head kernel AND bias uniform(1e-3) actor / uniform(3e-3) critic
    pa, pc = om.unflatten(a, sr.actor_shapes(cfg)), om.unflatten(c, sr.critic_shapes(cfg))
    for p, bound, fan0 in ((pa, 1e-3, 49), (pc, 3e-3, 53)):
        assert 0.5 * bound < np.abs(p["head_W"]).max() <= bound
        assert 0 < np.abs(p["head_b"]).max() <= bound  # (the critic's has two elements: no lower bar)
        assert np.all(p["b0"] == 0) and np.all(p["b2"] == 0)
        assert 0.9 * np.sqrt(6 / fan0) < np.abs(p["W0"]).max() <= np.sqrt(6 / fan0)
        assert 0.9 * np.sqrt(6 / 400) < np.abs(p["W1"]).max() <= np.sqrt(6 / 400)


def test_tie_and_untie():
    cfg = _cfg(3)
    st = sr.initialize(cfg, 4)
    for flat, shv, shm in ((st.actor, sr.actor_shapes(cfg), om.actor_leaf_shapes(cfg)),
                           (st.critic, sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg))):
        tied = om.unflatten(sr.tie(flat, shv, shm, 3), shm)
        v = om.unflatten(flat, shv)
        ax = 1 if tied["b0"].ndim == 2 else 0
        for t in range(3):
            np.testing.assert_array_equal(np.take(tied["head_W"], t, axis=ax), v["head_W"])
            np.testing.assert_array_equal(np.take(tied["head_b"], t, axis=ax), v["head_b"])
        np.testing.assert_array_equal(tied["W1"], v["W1"])
        back = om.unflatten(sr.untie_grad(sr.tie(flat, shv, shm, 3), shv, shm), shv)
        np.testing.assert_array_equal(back["head_W"], 3 * v["head_W"])  # the blocks are summed
        np.testing.assert_array_equal(back["W0"], v["W0"])


def test_per_task_gradients_average_to_the_step_gradient_parts():
    """With equal row counts the mean of the per-task critic gradients of the plain split losses is the full critic
    gradient only when the "next" actions are drawn at s' -- the task-gradient pass draws them at s, so what is
    held here is structural: every row's head columns are filled, and the head gradient of row t is the tied block t."""
    T, n = 3, 4
    cfg = _cfg(T)
    st = sr.initialize(cfg, 5, head_bound=1.0)
    batch = synthetic_batch(T, n * T, seed=3)
    en, ec = synthetic_eps(n * T, seed=4)
    Gc, Ga = sr.task_grads(cfg, st, batch, en, ec)
    assert Gc.shape == (T, st.critic.size) and Ga.shape == (T, st.actor.size)
    from oracle import conflict as oc

    Gm, _ = oc.task_grads(cfg, sr.tied_state(cfg, st), batch, en, ec)
    csh = om.critic_leaf_shapes(cfg)
    for t in range(T):
        mh = om.unflatten(Gm[t], csh)
        v = om.unflatten(Gc[t], sr.critic_shapes(cfg))
        np.testing.assert_array_equal(v["head_W"], mh["head_W"][:, t])
        for u in range(T):
            if u != t:
                assert np.all(mh["head_W"][:, u] == 0)
        assert np.count_nonzero(v["head_W"]) > v["head_W"].size // 2  # (a dead ReLU unit leaves a zero)


def test_a_dropped_task_in_the_head_sum_is_rejected_by_the_gpu_bars():
    """The seeded error (one task's block left out of the head gradient's sum) against the correct step, under the
    bars tests/test_gpu_shared_head_update.py applies: it must miss them."""
    T, n, W, A, E = 3, 8, 36, 1, 1
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A, num_critics=E)
    st = sr.initialize(cfg, seed=11)
    batch = synthetic_batch(T, n * T, action_dim=A, seed=100)
    en, ec = synthetic_eps(n * T, action_dim=A, seed=200)
    good, lg, ig = sr.update(cfg, st, batch, en, ec)
    bad, lb, ib = sr.update(cfg, st, batch, en, ec, skip_task=1)
    NORM_RTOL = 1e-4
    missed_norm = [k for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude")
                   if not abs(lb[k] - lg[k]) < NORM_RTOL * abs(lg[k])]
    assert missed_norm, (lb, lg)
    # the losses of the NEXT step move too (the critic was updated with a wrong head gradient): 1e-5 relative misses
    batch2 = synthetic_batch(T, n * T, action_dim=A, seed=101)
    en2, ec2 = synthetic_eps(n * T, action_dim=A, seed=201)
    l_good, l_bad = sr.update(cfg, good, batch2, en2, ec2)[1], sr.update(cfg, bad, batch2, en2, ec2)[1]
    assert any(abs(l_bad[k] - l_good[k]) > 1e-5 * abs(l_good[k]) for k in ("losses/qf_loss", "losses/actor_loss"))
    # and the per-element weight-grad bar of the kernel test (sum_bound(c_dot(B), S)): the dropped block is far outside
    import sac_head_ref as R

    gW_good = om.unflatten(ig["critic_grad"], sr.critic_shapes(cfg))["head_W"]
    gW_bad = om.unflatten(ib["critic_grad"], sr.critic_shapes(cfg))["head_W"]
    S = np.abs(gW_good) + np.abs(gW_bad)  # not below the exact sum of |terms| of either
    assert not R.within(gW_bad, gW_good, R.sum_bound(R.c_dot(n * T), S))


def test_trainer_refuses_what_the_shared_head_does_not_run():
    """MTSAC.initialize(shared_head=True): both networks must be plain VanillaNetworkConfig; no device call is made
    before the checks (this test runs without a GPU)."""
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig, VanillaNetworkConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.envs import MetaworldConfig
    from mtrl.rl.algorithms import MTSACConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    env = MetaworldConfig(env_id="MT10", terminate_on_success=False, reward_func_version="v2")
    opt = OptimizerConfig(max_grad_norm=1.0)

    def algo(net_a, net_c):
        return MTSACConfig(num_tasks=10, gamma=0.99, actor_config=ContinuousActionPolicyConfig(network_config=net_a),
                           critic_config=QValueFunctionConfig(network_config=net_c), num_critics=2)

    van = VanillaNetworkConfig(width=32, optimizer=opt)
    mh = MultiHeadConfig(width=32, num_tasks=10, optimizer=opt)
    for a, c, what in ((mh, van, "actor"), (van, mh, "critic"), (mh, mh, "actor")):
        with pytest.raises(NotImplementedError, match=f"{what}: shared_head runs the VanillaNetworkConfig"):
            MTSAC.initialize(algo(a, c), env, seed=1, shared_head=True)
    with pytest.raises(NotImplementedError, match="use_skip_connections"):
        MTSAC.initialize(algo(VanillaNetworkConfig(width=32, optimizer=opt, use_skip_connections=True), van), env,
                         seed=1, shared_head=True)
    with pytest.raises(NotImplementedError, match="use_layer_norm"):
        MTSAC.initialize(algo(van, VanillaNetworkConfig(width=32, optimizer=opt, use_layer_norm=True)), env, seed=1,
                         shared_head=True)


def test_environment_switch_is_read_when_shared_head_is_none(monkeypatch):
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.envs import MetaworldConfig
    from mtrl.rl.algorithms import MTSACConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    env = MetaworldConfig(env_id="MT10", terminate_on_success=False, reward_func_version="v2")
    mh = MultiHeadConfig(width=32, num_tasks=10, optimizer=OptimizerConfig(max_grad_norm=1.0))
    cfg = MTSACConfig(num_tasks=10, gamma=0.99, actor_config=ContinuousActionPolicyConfig(network_config=mh),
                      critic_config=QValueFunctionConfig(network_config=mh), num_critics=2)
    monkeypatch.setenv("MTSAC_VANILLA_SHARED_HEAD", "1")
    with pytest.raises(NotImplementedError, match="shared_head runs the VanillaNetworkConfig"):
        MTSAC.initialize(cfg, env, seed=1)  # None -> the environment says on -> MultiHead configs are refused


def test_checkpoint_tree_paths():
    from mtrl_amd import _lib as L
    from mtrl_amd.compat import checkpoint as C

    kw = dict(num_tasks=3, obs_dim=42, action_dim=4, actor_width=8, actor_depth=2, critic_width=8, critic_depth=3,
              num_critics=2, actor_max_grad_norm=1.0, critic_max_grad_norm=1.0, alpha_max_grad_norm=None)
    ash, csh = C.network_shapes(kw, "actor", True), C.network_shapes(kw, "critic", True)
    rng = np.random.default_rng(0)
    vec = {w: rng.standard_normal(sum(int(np.prod(s)) for _, s in (ash if w in (L.ACTOR, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU)
                                                                    else csh))).astype(np.float32)
           for w in (L.ACTOR, L.CRITIC, L.CRITIC_TARGET, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU, L.CRITIC_ADAM_MU, L.CRITIC_ADAM_NU)}
    for w in (L.LOG_ALPHA, L.ALPHA_ADAM_MU, L.ALPHA_ADAM_NU):
        vec[w] = rng.standard_normal(3).astype(np.float32)
    tree = C.agent_tree(kw, lambda w: vec[w], lambda i: 7 + i, shared_head=True)
    a_root, c_root = "params/VanillaNetwork_0/MLP_0", "params/VmapQValueFunction_0/VanillaNetwork_0/MLP_0"
    want = set()
    for i in range(3):  # actor: layer_0, layer_1 and the head layer_2
        want |= {f"actor/params/{a_root}/layer_{i}/{k}" for k in ("bias", "kernel")}
        want |= {f"actor/opt_state/1/0/{m}/{a_root}/layer_{i}/{k}" for m in ("mu", "nu") for k in ("bias", "kernel")}
    for i in range(4):
        for top in ("params", "target_params"):
            want |= {f"critic/{top}/{c_root}/layer_{i}/{k}" for k in ("bias", "kernel")}
        want |= {f"critic/opt_state/1/0/{m}/{c_root}/layer_{i}/{k}" for m in ("mu", "nu") for k in ("bias", "kernel")}
    got = {k for k in tree if "MLP_0" in k}
    assert got == want, (sorted(got ^ want))
    assert not any("MultiHeadNetwork_0" in k or "VmapDense_0" in k for k in tree)
    assert tree[f"actor/params/{a_root}/layer_2/kernel"].shape == (8, 8)  # (W, hd = 2 A)
    assert tree[f"critic/params/{c_root}/layer_3/kernel"].shape == (2, 8, 1)
    assert tree[f"critic/params/{c_root}/layer_3/bias"].shape == (2, 1)
    # the flat vector is the ravel order of this tree (keys sorted): layer_0 .. layer_D, the head last
    keys = sorted(k for k in tree if k.startswith(f"critic/params/{c_root}/"))
    np.testing.assert_array_equal(np.concatenate([tree[k].reshape(-1) for k in keys]), vec[L.CRITIC])
    # and back
    out = {}
    C.load_agent_tree(kw, tree, lambda w, v: out.__setitem__(w, np.asarray(v)), lambda i, n: None, shared_head=True)
    for w, v in vec.items():
        np.testing.assert_array_equal(out[w], v)
    # the multi-head tree is what it was
    mh = C.agent_tree(kw, lambda w: np.zeros(C_size(kw, w, C, L), np.float32), lambda i: 0)
    assert any("MultiHeadNetwork_0/VmapDense_0/kernel" in k for k in mh) and not any("MLP_0" in k for k in mh)


def C_size(kw, w, C, L):
    if w in (L.LOG_ALPHA, L.ALPHA_ADAM_MU, L.ALPHA_ADAM_NU):
        return kw["num_tasks"]
    sh = C.network_shapes(kw, "actor" if w in (L.ACTOR, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU) else "critic")
    return sum(int(np.prod(s)) for _, s in sh)


def test_shard_split_refuses_a_shared_head():
    from mtrl_amd import _lib as L
    from mtrl_amd.shard import shard_tasks

    with pytest.raises(L.MTSACError, match="-95"):
        shard_tasks(10, 2, 0, shared_head=True)
    assert shard_tasks(10, 2, 1) == (5, 5) and shard_tasks(10, 1, 0, shared_head=True) == (0, 10)
