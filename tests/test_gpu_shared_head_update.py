"""The shared-head (Vanilla) network on the MTSAC engine (MTSAC_NET_SHARED_HEAD) in every step form, against the
float64 step of tests/shared_head_ref.py.

Bars (those of tests/test_gpu_update.py and tests/test_gpu_optimizer.py): losses within 1e-5 relative, norms
within 1e-4; parameters after the steps by test_gpu_update's element bars (median 1e-6, max 2 lr steps + 1e-6);
the first step's parameters and moments from a mid-training state by the rule of tests/adam_ref.py -- the
engine's own gradient (read back from probe runs: a step from zero moments leaves mu' = (1 - b1) g) through the
float64 optimizer, allowed 4 times the numpy float32 yardstick's error in units of 2^-24 of each formula's
absolute terms.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import adam_ref as ar
import pcgrad_oracle as po
import shared_head_ref as sr
from helpers import synthetic_batch, synthetic_eps
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL, NORM_RTOL = 1e-5, 1e-4
PREC = {"fp32": 0, "split3": 1, "split2h": 3}
SHAPES = {"t1": (1, 5, 36, 4, 2), "t3": (3, 8, 36, 1, 1), "t4": (4, 5, 260, 6, 3)}  # (T, n, W, A, E)
K0 = 5  # Adam counts of the mid-training state


def _cfg(T, W, A, E, **kw):
    return om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A, num_critics=E, **kw)


def _engine(cfg, n, precision=0, shared=True, capacity=64, task_count=None, clips=True, **kw):
    from mtrl_amd.engine import MTSACEngine, make_config

    c = make_config(
        precision=precision, num_tasks=cfg.num_tasks, task_count=task_count or cfg.num_tasks, obs_dim=cfg.obs_dim,
        action_dim=cfg.action_dim, actor_width=cfg.actor_width, actor_depth=cfg.actor_depth,
        critic_width=cfg.critic_width, critic_depth=cfg.critic_depth, num_critics=cfg.num_critics, batch_per_task=n,
        capacity=capacity, gamma=cfg.gamma, tau=cfg.tau, clip=int(cfg.clip), use_task_weights=int(cfg.use_task_weights),
        actor_max_grad_norm=cfg.actor_max_grad_norm if clips in (True, "critic") else None,
        critic_max_grad_norm=cfg.critic_max_grad_norm if clips else None, **kw)
    e = MTSACEngine(c, shared_head=shared)
    e.enable_graph(False)
    return e


def _ids():
    from mtrl_amd import _lib as L

    return dict(actor=(L.ACTOR, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU), critic=(L.CRITIC, L.CRITIC_ADAM_MU, L.CRITIC_ADAM_NU),
                target=L.CRITIC_TARGET, alpha=L.LOG_ALPHA)


def _load(eng, st, moments=True):
    ids = _ids()
    eng.set_params(ids["actor"][0], st.actor)
    eng.set_params(ids["critic"][0], st.critic)
    eng.set_params(ids["target"], st.critic_target)
    eng.set_params(ids["alpha"], st.log_alpha)
    if moments:
        for net, opt in (("actor", st.actor_opt), ("critic", st.critic_opt)):
            eng.set_params(ids[net][1], opt.mu)
            eng.set_params(ids[net][2], opt.nu)
        eng.set_adam_count(0, st.actor_opt.count)
        eng.set_adam_count(1, st.critic_opt.count)


@functools.lru_cache(maxsize=None)
def _mid_state(name, head_bound=None, seed=11):
    """A mid-training state: parameters rounded through float32, Adam moments as K0 steps leave them (reachable,
    adam_ref.reachable_moments: the split2h planes' bound holds for those only), counts K0."""
    T, n, W, A, E = SHAPES[name]
    cfg = _cfg(T, W, A, E)
    st = sr.initialize(cfg, seed=seed, head_bound=head_bound)
    hp = ar.Hyper()
    for k, (net, opt) in enumerate((("actor", st.actor_opt), ("critic", st.critic_opt))):
        mu, nu = ar.reachable_moments(np.full(getattr(st, net).size, 2e-3), hp, seed + k, steps=K0)
        opt.mu, opt.nu, opt.count = mu.astype(np.float64), nu.astype(np.float64), K0
    st.critic_target = (st.critic + 1e-3 * np.random.default_rng(seed).standard_normal(st.critic.size)).astype(
        np.float32).astype(np.float64)
    return cfg, st


@functools.lru_cache(maxsize=None)
def _ref_run(name, steps=3):
    """The reference steps, once per shape, shared by the precisions and never mutated."""
    T, n, W, A, E = SHAPES[name]
    cfg, st = _mid_state(name)
    out = []
    for k in range(steps):
        batch = synthetic_batch(T, n * T, action_dim=A, seed=100 + k, dtype=np.float32)
        en, ec = synthetic_eps(n * T, action_dim=A, seed=200 + k, dtype=np.float32)
        st, logs, _ = sr.update(cfg, st, batch, en.astype(np.float64), ec.astype(np.float64))
        out.append((batch, en, ec, logs))
    return cfg, st, out


def _check_logs(got, want, tag, alpha_zero=False):
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values"):
        if k == "losses/alpha_loss" and alpha_zero:
            assert abs(got[k]) < 1e-6  # log_alpha = 0: the loss is exactly 0
            continue
        scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
        assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (tag, k, got[k], want[k])
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
              "metrics/actor_params_norm", "alpha"):
        assert abs(got[k] - want[k]) < NORM_RTOL * abs(want[k]), (tag, k, got[k], want[k])


def _check_state(eng, st, steps, tag):
    ids = _ids()
    for which, ref in ((ids["actor"][0], st.actor), (ids["critic"][0], st.critic), (ids["target"], st.critic_target),
                       (ids["alpha"], st.log_alpha), (ids["actor"][1], st.actor_opt.mu), (ids["critic"][1], st.critic_opt.mu),
                       (ids["actor"][2], st.actor_opt.nu), (ids["critic"][2], st.critic_opt.nu)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (tag, which, np.median(d))
        assert d.max() < 2 * 3e-4 * steps + 1e-6, (tag, which, d.max())


def _adam_rule(name, pname, batch, en, ec):
    """The first step's mu', nu', p' (target') of both networks by adam_ref's rule, on the engine's own gradient."""
    T, n, W, A, E = SHAPES[name]
    cfg, st = _mid_state(name)
    ids, hp = _ids(), ar.Hyper()
    b1 = float(np.float32(1) - np.float32(hp.b1))

    def run(critic_state, actor_state, clips):
        eng = _engine(cfg, n, PREC[pname], clips=clips)
        s = st.copy()
        if not critic_state:
            s.critic_opt = om.AdamState.zeros(st.critic.size, np.float64)
        if not actor_state:
            s.actor_opt = om.AdamState.zeros(st.actor.size, np.float64)
        _load(eng, s)
        eng.update(batch, en, ec)
        out = {net: [eng.get_params(i) for i in ids[net]] for net in ("actor", "critic")}
        out["target"] = eng.get_params(ids["target"])
        eng.close()
        return out

    g_c = run(False, False, False)["critic"][1].astype(np.float64) / b1
    # the actor is differentiated through the UPDATED critic: the critic exactly as in the run, the actor from zero
    probe_b = run(True, False, "critic")  # (the critic's clip as in the run, none on the actor)
    got = run(True, True, True)
    fails = []
    ref, lo, S, c = ar.yardstick(st.critic, g_c, st.critic_opt.mu, st.critic_opt.nu, K0, hp, cfg.critic_max_grad_norm,
                                 st.critic_target)
    for q, arr in (("mu", got["critic"][1]), ("nu", got["critic"][2]), ("p", got["critic"][0]), ("target", got["target"])):
        r = ar.units(arr, getattr(ref, q), S[q])
        print(f"{name} {pname} critic {q}': engine {r:.2f} yardstick {c[q]:.2f} units")
        if not r <= 4 * c[q]:
            fails.append(("critic", q, r, c[q]))
    g_a = probe_b["actor"][1].astype(np.float64) / b1
    ref, lo, S, c = ar.yardstick(st.actor, g_a, st.actor_opt.mu, st.actor_opt.nu, K0, hp, cfg.actor_max_grad_norm)
    for q, arr in (("mu", got["actor"][1]), ("nu", got["actor"][2]), ("p", got["actor"][0])):
        r = ar.units(arr, getattr(ref, q), S[q])
        print(f"{name} {pname} actor {q}': engine {r:.2f} yardstick {c[q]:.2f} units")
        if not r <= 4 * c[q]:
            fails.append(("actor", q, r, c[q]))
    assert not fails, fails


@pytest.mark.parametrize("pname", list(PREC))
@pytest.mark.parametrize("name", list(SHAPES))
def test_three_steps_match_the_reference(name, pname):
    T, n, W, A, E = SHAPES[name]
    cfg, st_end, steps = _ref_run(name)
    _, st0 = _mid_state(name)
    eng = _engine(cfg, n, PREC[pname])
    assert eng.lib.mtsac_shared_head(eng._h) == 1
    assert eng.param_count(0) == sr.param_count(cfg.actor_in, W, cfg.actor_depth, 2 * A) == st0.actor.size
    assert eng.param_count(1) == sr.param_count(cfg.critic_in, W, cfg.critic_depth, 1, E) == st0.critic.size
    _load(eng, st0)
    for k, (batch, en, ec, want) in enumerate(steps):
        eng.update(batch, en, ec)
        got = eng.logs()
        _check_logs(got, want, (name, pname, k), alpha_zero=(k == 0))
        assert got["metrics/explore_loss"] == 0.0
    _check_state(eng, st_end, len(steps), (name, pname))
    assert [eng.get_adam_count(i) for i in range(3)] == [K0 + 3, K0 + 3, 3]
    eng.close()
    _adam_rule(name, pname, *steps[0][:3])


@pytest.mark.parametrize("pname", list(PREC))
def test_one_task_shared_head_is_the_multi_head_engine(pname):
    """T = 1: one head either way.  Same values -> same logs and parameters within the bars (the head's gradient
    comes from another kernel, so not bitwise)."""
    name = "t1"
    T, n, W, A, E = SHAPES[name]
    cfg, st = _mid_state(name)
    mh = sr.tied_state(cfg, st)
    mh.actor_opt = om.AdamState(sr.tie(st.actor_opt.mu, sr.actor_shapes(cfg), om.actor_leaf_shapes(cfg), 1),
                                sr.tie(st.actor_opt.nu, sr.actor_shapes(cfg), om.actor_leaf_shapes(cfg), 1), K0)
    mh.critic_opt = om.AdamState(sr.tie(st.critic_opt.mu, sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg), 1),
                                 sr.tie(st.critic_opt.nu, sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg), 1), K0)
    outs = []
    for shared, s in ((True, st), (False, mh)):
        eng = _engine(cfg, n, PREC[pname], shared=shared)
        _load(eng, s)
        logs = []
        for k in range(3):
            batch = synthetic_batch(T, n * T, action_dim=A, seed=300 + k, dtype=np.float32)
            en, ec = synthetic_eps(n * T, action_dim=A, seed=400 + k, dtype=np.float32)
            eng.update(batch, en, ec)
            logs.append(eng.logs())
        ids = _ids()
        outs.append((logs, eng.get_params(ids["actor"][0]), eng.get_params(ids["critic"][0])))
        eng.close()
    for k in range(3):
        _check_logs(outs[0][0][k], outs[1][0][k], (pname, k), alpha_zero=(k == 0))
    for w, (shv, shm) in enumerate(((sr.actor_shapes(cfg), om.actor_leaf_shapes(cfg)),
                                    (sr.critic_shapes(cfg), om.critic_leaf_shapes(cfg)))):
        d = np.abs(sr.tie(outs[0][1 + w].astype(np.float64), shv, shm, 1) - outs[1][1 + w])
        assert np.median(d) < 1e-6 and d.max() < 2 * 3e-4 * 3 + 1e-6, (pname, w, d.max())


def _snapshot(eng):
    return [eng.get_params(w) for w in range(10)] + [np.array(list(eng.logs().values()))]


@pytest.mark.parametrize("pname", ["fp32", "split2h"])
@pytest.mark.parametrize("form", ["graph", "pipelined"])
def test_update_many_equals_eager_updates_bitwise(form, pname):
    """update_many(3) under hipGraph replay, and on the pipelined lanes, against three eager one-step calls."""
    name = "t3"
    T, n, W, A, E = SHAPES[name]
    cfg, st = _mid_state(name)
    outs = []
    for mode in ("eager", form):
        eng = _engine(cfg, n, PREC[pname])
        if mode == "pipelined":
            eng.lib.mtsac_debug_set_pipeline(eng._h, 1)
        _load(eng, st)
        eng.buffer_fill_synthetic(99)
        eng.seed_rng(1)
        eng.enable_graph(mode == "graph")
        if mode == "eager":
            for _ in range(3):
                eng.update_many(1)
        else:
            eng.update_many(3)
        outs.append(_snapshot(eng))
        eng.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_compacted_and_dense_actor_pass_agree_bitwise():
    """split2h, two critics, the shape of tests/test_gpu_actor_compact.py (where the ragged data grads run): the
    compacted actor pass runs with a shared head and leaves the dense pass's bits."""
    from mtrl_amd import _lib as L
    from mtrl_amd.init import init_vanilla

    T, n, W, A, E = 20, 128, 2048, 4, 2
    cfg = _cfg(T, W, A, E)
    actor, critic = init_vanilla(T, 39 + T, A, W, 3, W, 3, E, seed=1)
    outs, ran = [], []
    lib = L.load()
    for dense in (0, 1):
        L.check(lib.mtsac_debug_set_actor_dense(dense))  # read at engine creation
        try:
            eng = _engine(cfg, n, PREC["split2h"], capacity=512)
        finally:
            L.check(lib.mtsac_debug_set_actor_dense(-1))
        eng.set_params(L.ACTOR, actor)
        eng.set_params(L.CRITIC, critic)
        eng.set_params(L.CRITIC_TARGET, critic)
        eng.buffer_fill_synthetic(7)
        eng.seed_rng(2)
        eng.update_many(2)
        ran.append(lib.mtsac_debug_actor_compact(eng._h))
        outs.append(_snapshot(eng))
        eng.close()
    assert ran == [1, 0], ("the compacted pass must run in the first engine and not in the second", ran)
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_clip_and_task_weights_in_the_plain_step():
    T, n, W, A, E = SHAPES["t3"]
    cfg = _cfg(T, W, A, E, clip=True, use_task_weights=True)
    st = sr.initialize(cfg, seed=5)
    st.log_alpha = np.array([0.25, -0.5, 0.125])
    eng = _engine(cfg, n, 0)
    _load(eng, st, moments=False)
    for k in range(2):
        batch = synthetic_batch(T, n * T, action_dim=A, seed=500 + k, dtype=np.float32)
        en, ec = synthetic_eps(n * T, action_dim=A, seed=600 + k, dtype=np.float32)
        st, want, _ = sr.update(cfg, st, batch, en.astype(np.float64), ec.astype(np.float64))
        eng.update(batch, en, ec)
        _check_logs(eng.logs(), want, ("clip_tw", k))
    eng.close()


def test_device_noise_steps_are_reproducible_and_bf16_runs():
    T, n, W, A, E = SHAPES["t3"]
    cfg, st = _mid_state("t3")
    outs = []
    for _ in range(2):
        eng = _engine(cfg, n, 0)
        _load(eng, st)
        batch = synthetic_batch(T, n * T, action_dim=A, seed=700, dtype=np.float32)
        eng.update(batch)  # no eps: the device noise stream
        outs.append(_snapshot(eng))
        eng.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    eng = _engine(cfg, n, 2)  # precision bf16 (perf-only arithmetic: finite logs, counts advance)
    _load(eng, st)
    eng.buffer_fill_synthetic(3)
    eng.update_many(2)
    assert all(np.isfinite(v) for v in eng.logs().values()) and eng.get_adam_count(1) == K0 + 2
    eng.close()


def test_rollout_actions_and_param_round_trip():
    name = "t4"
    T, n, W, A, E = SHAPES[name]
    cfg, st = _mid_state(name)
    eng = _engine(cfg, n, 0)
    _load(eng, st)
    ids = _ids()
    for which, ref in ((ids["actor"][0], st.actor), (ids["critic"][0], st.critic), (ids["target"], st.critic_target),
                       (ids["actor"][1], st.actor_opt.mu), (ids["critic"][2], st.critic_opt.nu)):
        np.testing.assert_array_equal(eng.get_params(which).view(np.uint32), ref.astype(np.float32).view(np.uint32))
    # the Vanilla order: writing a vector that counts its own elements comes back as it went in
    ramp = np.arange(st.critic.size, dtype=np.float32)
    eng.set_params(ids["critic"][1], ramp)
    np.testing.assert_array_equal(eng.get_params(ids["critic"][1]), ramp)
    obs = synthetic_batch(T, 2 * T, action_dim=A, seed=3, dtype=np.float32)[0]
    eps = np.random.default_rng(4).standard_normal((2 * T, A)).astype(np.float32)
    np.testing.assert_allclose(eng.eval_action(obs), sr.eval_action(cfg, st, obs), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(eng.sample_action(obs, eps), sr.sample_action(cfg, st, obs, eps), rtol=1e-5, atol=1e-6)
    eng.close()


def test_sharded_config_is_refused():
    from mtrl_amd import _lib as L
    from mtrl_amd.shard import shard_tasks

    cfg = _cfg(4, 36, 4, 2)
    with pytest.raises(L.MTSACError, match="-95"):
        _engine(cfg, 4, 0, task_count=2)
    with pytest.raises(L.MTSACError, match="-95"):
        shard_tasks(4, 2, 0, shared_head=True)
    assert shard_tasks(4, 1, 0, shared_head=True) == (0, 4)
    eng = _engine(cfg, 4, 0)
    with pytest.raises(L.MTSACError, match="-95"):
        eng.set_allreduce_hook(lambda ptr, count: None)
    eng.close()


# ------------------------------------------------------------------ per-task gradients and the surgery steps
def _noise(rng, n, T, A):
    return np.repeat(rng.standard_normal((n, A)), T, axis=0).astype(np.float32)  # rows i*T + t share draw i


def _rows_bound(G):
    """Per-element bar of a [T][P] gradient matrix against float64: 1e-5 of the row's largest magnitude (the bar
    tests/test_gpu_conflict.py holds the multi-head matrices to is relative to the row's scale)."""
    return 1e-5 * np.abs(G).max(axis=1, keepdims=True) + 1e-9


def test_task_gradients_match_the_reference():
    T, n, W, A, E = 3, 8, 36, 4, 2
    cfg = _cfg(T, W, A, E)
    st = sr.initialize(cfg, seed=9, head_bound=1.0)
    batch = list(synthetic_batch(T, n * T, action_dim=A, seed=800, dtype=np.float32))
    rng = np.random.default_rng(1)
    en, ec = _noise(rng, n, T, A), _noise(rng, n, T, A)
    eng = _engine(cfg, n, 0)
    _load(eng, st, moments=False)
    eng.task_gradients(tuple(batch), en, ec)
    Gc, Ga = eng.get_task_gradients(0), eng.get_task_gradients(1)
    want_c, want_a = sr.task_grads(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64),
                                   ec.astype(np.float64))
    assert Gc.shape == want_c.shape == (T, st.critic.size) and Ga.shape == want_a.shape == (T, st.actor.size)
    for got, want in ((Gc, want_c), (Ga, want_a)):
        assert np.all(np.abs(got - want) <= _rows_bound(want)), np.abs(got - want).max()
    # the shared head makes the tasks' head gradients overlap (a multi-head matrix has disjoint head blocks)
    hW = sr.critic_shapes(cfg)[-1][1]
    assert np.count_nonzero(np.all(want_c[:, -int(np.prod(hW)):] != 0, axis=0)) > 0
    # select and stats run on the matrix
    ranks = np.tile(np.array([0, st.critic.size - 1], np.int64), (T, 1))
    v = eng.task_gradient_select(0, ranks)
    a = np.sort(np.abs(Gc), axis=1)
    np.testing.assert_array_equal(v, np.stack([a[:, 0], a[:, -1]], axis=1))
    stt = eng.task_gradient_stats(0, np.zeros(T, np.float32), 1e-3, 1.0)
    gram = Gc.astype(np.float64) @ Gc.astype(np.float64).T
    np.testing.assert_allclose(stt["gram"], gram, rtol=2e-6, atol=1e-6 * np.abs(gram).max())  # test_gpu_conflict's bar
    eng.close()


def test_task_gradients_with_a_task_whose_dq_is_zero():
    """clip = True and task 1's observations scaled until every Q of its rows lies beyond +-5000: the clip's
    derivative is 0 there, so dq is exactly zero on all of task 1's rows and its row of the critic matrix is
    exactly zero -- head columns included -- while the other tasks' rows keep the reference's values."""
    T, n, W, A, E = 3, 4, 36, 4, 2
    cfg = _cfg(T, W, A, E, clip=True)
    st = sr.initialize(cfg, seed=10, head_bound=1.0)
    batch = [b.copy() for b in synthetic_batch(T, n * T, action_dim=A, seed=801, dtype=np.float32)]
    rows = np.flatnonzero(np.arange(n * T) % T == 1)
    batch[0][rows, :39] *= np.float32(2.0 ** 20)
    rng = np.random.default_rng(2)
    en, ec = _noise(rng, n, T, A), _noise(rng, n, T, A)
    want_c, _ = sr.task_grads(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64), ec.astype(np.float64))
    assert np.all(want_c[1] == 0) and np.abs(want_c[0]).max() > 0, "the case must zero task 1's dq"
    eng = _engine(cfg, n, 0)
    _load(eng, st, moments=False)
    eng.task_gradients(tuple(batch), en, ec)
    Gc = eng.get_task_gradients(0)
    assert np.all(Gc[1] == 0), np.abs(Gc[1]).max()
    for t in (0, 2):
        assert np.all(np.abs(Gc[t] - want_c[t]) <= _rows_bound(want_c[t:t + 1])[0]), t
    eng.close()


def _surgery_case(seed):
    T, n, W, A, E = 3, 8, 36, 4, 2
    cfg = _cfg(T, W, A, E)
    st = sr.initialize(cfg, seed=seed, head_bound=1.0)
    batch = synthetic_batch(T, n * T, action_dim=A, seed=seed + 100, dtype=np.float32)
    rng = np.random.default_rng(seed + 7)
    return cfg, st, n, batch, _noise(rng, n, T, A), _noise(rng, n, T, A)


def _check_surgery_step(eng, st_new, want, extra=()):
    got = eng.logs()
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/qf_values", "metrics/explore_loss"):
        scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
        assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (k, got[k], want[k])
    assert abs(got["losses/alpha_loss"]) < 1e-6
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
              "metrics/actor_params_norm", "alpha"):
        assert abs(got[k] - want[k]) < NORM_RTOL * abs(want[k]), (k, got[k], want[k])
    _check_state(eng, st_new, 1, "surgery")


def test_cagrad_step_matches_the_oracle_on_shared_head_gradients():
    from mtrl_amd.cagrad import cagrad_direct

    cfg, st, n, batch, en, ec = _surgery_case(23)
    eng = _engine(cfg, n, 1)
    eng.set_cagrad(True)
    _load(eng, st, moments=False)
    lg = {}
    st1, want, _ = sr.surgery_update(
        cfg, st, batch, en.astype(np.float64), ec.astype(np.float64),
        lambda G, L: lg.setdefault("c", cagrad_direct(G))[0], lambda G, L: lg.setdefault("a", cagrad_direct(G))[0])
    want["metrics/critic_grad_magnitude"] = lg["c"][1]["grad_magnitude"]
    want["metrics/actor_grad_magnitude"] = lg["a"][1]["grad_magnitude"]
    eng.update(batch, en, ec)
    _check_surgery_step(eng, st1, want)
    ca = eng.cagrad_logs()
    for net, key in (("critic", "c"), ("actor", "a")):
        for k in ("avg_grad_magnitude", "avg_grad_magnitude_before_surgery", "cagrad_objective"):
            g, w = ca[f"metrics/{net}_{k}"], lg[key][1][k]
            assert abs(g - w) <= NORM_RTOL * abs(w), (net, k, g, w)
    eng.close()


def test_gradnorm_step_matches_the_oracle_on_shared_head_gradients():
    from mtrl_amd.gradnorm import gradnorm_direct, gradnorm_init

    cfg, st, n, batch, en, ec = _surgery_case(29)
    T = cfg.num_tasks
    eng = _engine(cfg, n, 1)
    eng.set_gradnorm(True)
    _load(eng, st, moments=False)
    lg = {}
    st1, want, _ = sr.surgery_update(
        cfg, st, batch, en.astype(np.float64), ec.astype(np.float64),
        lambda G, L: lg.setdefault("c", gradnorm_direct(G, L, gradnorm_init(T)))[0],
        lambda G, L: lg.setdefault("a", gradnorm_direct(G, L, gradnorm_init(T)))[0])
    want["metrics/critic_grad_magnitude"] = lg["c"][2]["grad_magnitude"]
    want["metrics/actor_grad_magnitude"] = lg["a"][2]["grad_magnitude"]
    eng.update(batch, en, ec)
    _check_surgery_step(eng, st1, want)
    tl = eng.gradnorm_task_losses()
    np.testing.assert_allclose(tl[0], sr.critic_task_losses(cfg, st, batch, en.astype(np.float64)), rtol=1e-5)
    eng.close()


def test_pcgrad_step_with_a_pinned_order():
    cfg, st, n, batch, en, ec = _surgery_case(31)
    pc, pa = np.array([2, 0, 1], np.int32), np.array([1, 2, 0], np.int32)
    eng = _engine(cfg, n, 1)
    eng.set_pcgrad(True)
    eng.pcgrad_set_order(pc, pa)
    _load(eng, st, moments=False)
    margins = []

    def comb(perm):
        def f(G, L):
            g, _, m = po.surgery(G, perm)
            margins.append(m)
            return g
        return f

    st1, want, _ = sr.surgery_update(cfg, st, batch, en.astype(np.float64), ec.astype(np.float64), comb(pc), comb(pa))
    assert min(margins) > 1e-4, margins  # no projection decision hinges on rounding
    eng.update(batch, en, ec)
    _check_surgery_step(eng, st1, want)
    eng.close()


def test_compute_weights_and_network_metrics_key_sets():
    from mtrl_amd.conflict import compute_weights
    from mtrl_amd.netmetrics import expected_keys
    from mtrl.config.utils import Metrics
    from mtrl_amd.netmetrics import compute_metrics

    T, n, W, A, E = 3, 8, 36, 4, 2
    cfg = _cfg(T, W, A, E)
    st = sr.initialize(cfg, seed=12, head_bound=1.0)
    batch = synthetic_batch(T, n * T, action_dim=A, seed=900, dtype=np.float32)
    rng = np.random.default_rng(3)
    en, ec = _noise(rng, n, T, A), _noise(rng, n, T, A)
    keys = []
    for shared in (True, False):
        eng = _engine(cfg, n, 0, shared=shared)
        if shared:
            _load(eng, st, moments=False)
        logs = compute_weights(eng, tuple(batch), en, ec)
        keys.append(set(logs))
        if shared:
            assert all(np.all(np.isfinite(v)) for v in logs.values())
            m = compute_metrics(eng, Metrics.ALL, batch[0], ec)
            assert set(m) == set(expected_keys(cfg.actor_depth, cfg.critic_depth, E))
        eng.close()
    assert keys[0] == keys[1] and len(keys[0]) == 66


def test_trainer_runs_the_vanilla_tree_with_cagrad():
    """MTSAC.initialize(..., shared_head=True) with CAGrad on both networks (the reference's mt10_mtmhsac_cagrad.py
    network), after tests/test_gpu_cagrad.py test_trainer_with_cagrad_on_both_networks."""
    from fake_env import FakeMetaworldConfig, FakeMTVecEnv
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import VanillaNetworkConfig
    from mtrl.config.optim import CAGradConfig, OptimizerConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.rl.algorithms import MTSACConfig
    from mtrl.rl.algorithms.mtsac import MTSAC

    T, W = 3, 32

    class ThreeTasks(FakeMetaworldConfig):
        @property
        def num_tasks(self) -> int:
            return T

    opt = CAGradConfig(num_tasks=T, max_grad_norm=1.0, cagrad_optimizer=OptimizerConfig(max_grad_norm=1.0))
    algo = MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=VanillaNetworkConfig(width=W, optimizer=opt)),
        critic_config=QValueFunctionConfig(network_config=VanillaNetworkConfig(width=W, optimizer=opt)), num_critics=2)
    env_cfg = ThreeTasks(env_id="MT3")
    tc = OffPolicyTrainingConfig(total_steps=1000, buffer_size=50 * T, batch_size=8 * T, warmstart_steps=5,
                                 evaluation_frequency=10)
    agent = MTSAC.initialize(algo, env_cfg, seed=1, precision="split3", shared_head=True)
    assert agent.cagrad and agent.shared_head and agent.engine.shared_head
    D, A = 39 + T, 4
    assert agent.get_num_params() == {"actor_num_params": sr.param_count(D, W, 3, 2 * A),
                                      "critic_num_params": sr.param_count(D + A, W, 3, 1, 2)}
    buf = agent.spawn_replay_buffer(env_cfg, tc, 1)  # rebuilds the engine: the mode is kept
    assert agent.engine.shared_head and agent.engine.lib.mtsac_shared_head(agent.engine._h) == 1
    env = FakeMTVecEnv(T)
    obs, _ = env.reset()
    for _ in range(12):
        nobs, r, term, trunc, _ = env.step(env.action_space.sample())
        buf.add(obs, nobs, env.action_space.sample(), r, np.logical_or(term, trunc))
        obs = nobs
    for _ in range(3):
        agent, logs = agent.update_from_buffer(buf, tc.batch_size, want_logs=True)
        d = dict(logs)
        assert len(d) == 20
        assert all(np.isfinite(v) for k, v in d.items() if np.ndim(v) == 0 and "cosine" not in k)
    assert agent.engine.get_adam_count(0) == 3 and agent.engine.get_adam_count(1) == 3
    sd = agent.state_dict()
    assert f"actor/params/params/VanillaNetwork_0/MLP_0/layer_3/kernel" in sd
    assert sd["critic/target_params/params/VmapQValueFunction_0/VanillaNetwork_0/MLP_0/layer_3/kernel"].shape == (2, W, 1)
    before = agent.engine.get_params(1)
    agent.load_state_dict(sd)
    np.testing.assert_array_equal(agent.engine.get_params(1), before)
