"""The plain step on a device-sampled batch with per-task sizes (mtsac_set_task_batch_sizes), in every step form.

* Bitwise against mtsac_update on another engine fed the very rows, with the same injected noise: same kernels,
  same row lists, so logs, parameters, moments and target must have the same bits.
* Three steps from a mid-training state against the float64 oracle (oracle/mtsac.py reads each row's task from its
  one-hot, so it takes task-major batches with unequal counts as they are) on the rows numpy samples
  (tests/task_batch_cases.py), under the suite's bars and no new one: losses 1e-5 relative, norms 1e-4
  (tests/test_gpu_update.py), parameters after the steps median 1e-6 / max 2 lr steps + 1e-6, and the first step's
  parameters and moments by the rule of tests/adam_ref.py (the engine's own gradient from probe runs through the
  float64 optimizer, 4 times the numpy float32 yardstick's error).
* An empty task: its head gradients and its log_alpha gradient are exactly 0.
* update_many(k) = k eager updates, pipelined = eager, graph replay = eager, bitwise, new sizes mid-run included.
* The per-task losses against the oracle's per-row terms (1e-5 relative; 0 for an empty task), and the step's
  outputs with the reduction on and off.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import adam_ref as ar
import task_batch_cases as tc
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

LOSS_RTOL, NORM_RTOL = 1e-5, 1e-4
PREC = {"fp32": 0, "split3": 1, "split2h": 3}
K0 = 5  # Adam counts of the mid-training state
SEED = 17  # index stream


def _cfg(name, **kw):
    T, n, W, A, E = tc.SHAPES[name]
    return om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=W, critic_width=W, action_dim=A, num_critics=E, **kw)


def _engine(cfg, n, precision=0, clips=True, **kw):
    from mtrl_amd.engine import MTSACEngine, make_config

    c = make_config(
        precision=precision, num_tasks=cfg.num_tasks, task_count=cfg.num_tasks, obs_dim=cfg.obs_dim,
        action_dim=cfg.action_dim, actor_width=cfg.actor_width, actor_depth=cfg.actor_depth,
        critic_width=cfg.critic_width, critic_depth=cfg.critic_depth, num_critics=cfg.num_critics, batch_per_task=n,
        capacity=tc.CAPACITY, gamma=cfg.gamma, tau=cfg.tau,
        actor_max_grad_norm=cfg.actor_max_grad_norm if clips is True else None,  # clips "critic": the critic's only
        critic_max_grad_norm=cfg.critic_max_grad_norm if clips else None, **kw)
    e = MTSACEngine(c)
    e.enable_graph(False)
    return e


def _ids():
    from mtrl_amd import _lib as L

    return dict(actor=(L.ACTOR, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU), critic=(L.CRITIC, L.CRITIC_ADAM_MU, L.CRITIC_ADAM_NU),
                target=L.CRITIC_TARGET, alpha=(L.LOG_ALPHA, L.ALPHA_ADAM_MU, L.ALPHA_ADAM_NU))


def _load(eng, st):
    ids = _ids()
    eng.set_params(ids["target"], st.critic_target)
    for i, (net, p, opt) in enumerate((("actor", st.actor, st.actor_opt), ("critic", st.critic, st.critic_opt),
                                       ("alpha", st.log_alpha, st.alpha_opt))):
        eng.set_params(ids[net][0], p)
        eng.set_params(ids[net][1], opt.mu)
        eng.set_params(ids[net][2], opt.nu)
        eng.set_adam_count(i, opt.count)


@functools.lru_cache(maxsize=None)
def _mid_state(name, seed=11):
    """Parameters rounded through float32, hidden biases and log_alpha off zero, the target off the critic, Adam
    moments of actor and critic as K0 steps leave them (adam_ref.reachable_moments), counts K0."""
    cfg = _cfg(name)
    st = om.initialize(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for attr, shapes in (("actor", om.actor_leaf_shapes(cfg)), ("critic", om.critic_leaf_shapes(cfg))):
        p = om.unflatten(getattr(st, attr), shapes)
        for k in p:
            if k.startswith("b"):
                p[k] = rng.normal(0.0, 0.01, p[k].shape)
        setattr(st, attr, om.flatten(p, shapes).astype(np.float32).astype(np.float64))
    st.critic_target = (st.critic + rng.normal(0.0, 1e-3, st.critic.size)).astype(np.float32).astype(np.float64)
    st.log_alpha = rng.uniform(-0.3, 0.3, cfg.num_tasks).astype(np.float32).astype(np.float64)
    hp = ar.Hyper()
    for k, (net, opt) in enumerate((("actor", st.actor_opt), ("critic", st.critic_opt))):
        mu, nu = ar.reachable_moments(np.full(getattr(st, net).size, 2e-3), hp, seed + k, steps=K0)
        opt.mu, opt.nu, opt.count = mu.astype(np.float64), nu.astype(np.float64), K0
    return cfg, st


@functools.lru_cache(maxsize=None)
def _store(name):
    T, n, W, A, E = tc.SHAPES[name]
    return tc.make_store(T, A, tc.CAPACITY, seed=6, pin_max=True)


def _eps(name, k):
    T, n, W, A, E = tc.SHAPES[name]
    rng = np.random.default_rng(300 + k)
    return rng.standard_normal((n * T, A)).astype(np.float32), rng.standard_normal((n * T, A)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ref_run(name, sizes, steps=3):
    """The rows numpy samples and the float64 steps on them, once per case, shared by the precisions."""
    T, n, W, A, E = tc.SHAPES[name]
    cfg, st = _mid_state(name)
    rng = np.random.default_rng(SEED)
    out = []
    for k in range(steps):
        _, rows = tc.reference_sample(_store(name), rng, sizes, tc.CAPACITY, n * T)
        batch = rows[:5]
        en, ec = _eps(name, k)
        st, logs, internals = om.update(cfg, st, [b.astype(np.float64) for b in batch], en.astype(np.float64),
                                        ec.astype(np.float64), return_internals=True)
        out.append((batch, rows[5], en, ec, logs, internals))
    return cfg, st, out


def _sampling_engine(name, sizes, pname, st, **kw):
    """An engine at the state, its buffer filled and seeded, per-task sizes set."""
    T, n, W, A, E = tc.SHAPES[name]
    eng = _engine(_cfg(name), n, PREC[pname], **kw)
    _load(eng, st)
    tc.fill_engine(eng, _store(name))
    eng.seed_rng(SEED)
    if sizes is not None:
        eng.set_task_batch_sizes(np.array(sizes))
    return eng


def _snapshot(eng):
    return [eng.get_params(w) for w in range(10)] + [np.array(list(eng.logs().values()), np.float32)] + \
           [np.array([eng.get_adam_count(i) for i in range(3)], np.float32)]


def _assert_same_bits(a, b, tag):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (tag, i, int(np.sum(x != y)))


def _check_logs(got, want, tag):
    for k in ("losses/qf_loss", "losses/actor_loss", "losses/alpha_loss", "losses/qf_values"):
        scale = max(abs(want[k]), 1e-3) if k == "losses/qf_values" else abs(want[k])
        print(tag, k, got[k], want[k])
        assert abs(got[k] - want[k]) <= LOSS_RTOL * scale, (tag, k, got[k], want[k])
    for k in ("metrics/critic_grad_magnitude", "metrics/actor_grad_magnitude", "metrics/critic_params_norm",
              "metrics/actor_params_norm", "alpha"):
        print(tag, k, got[k], want[k])
        assert abs(got[k] - want[k]) < NORM_RTOL * abs(want[k]), (tag, k, got[k], want[k])


def _check_state(eng, st, steps, tag):
    ids = _ids()
    for which, ref in ((ids["actor"][0], st.actor), (ids["critic"][0], st.critic), (ids["target"], st.critic_target),
                       (ids["alpha"][0], st.log_alpha), (ids["actor"][1], st.actor_opt.mu),
                       (ids["critic"][1], st.critic_opt.mu), (ids["actor"][2], st.actor_opt.nu),
                       (ids["critic"][2], st.critic_opt.nu)):
        d = np.abs(eng.get_params(which).astype(np.float64) - ref)
        assert np.median(d) < 1e-6, (tag, which, np.median(d))
        assert d.max() < 2 * 3e-4 * steps + 1e-6, (tag, which, d.max())


# ------------------------------------------------------------------ device-sampled = the same rows fed by the user
@pytest.mark.parametrize("pname", list(PREC))
@pytest.mark.parametrize("name,sizes", tc.CASES, ids=tc.CASE_IDS)
def test_device_sampled_step_equals_user_batch_step_bitwise(name, sizes, pname):
    T, n, W, A, E = tc.SHAPES[name]
    _, st = _mid_state(name)
    sampler = _sampling_engine(name, sizes, pname, st)  # only samples: the rows of every step
    dev = _sampling_engine(name, sizes, pname, st)
    user = _sampling_engine(name, None, pname, st)
    for k in range(2):
        idx, rows = sampler.sample()
        np.testing.assert_array_equal(np.argmax(rows[0][:, 39:], axis=1), np.repeat(np.arange(T), sizes))
        en, ec = _eps(name, k)
        dev.update(None, en, ec)
        user.update(rows, en, ec)
        _assert_same_bits(_snapshot(dev), _snapshot(user), (name, sizes, pname, k))
        assert dev.get_rng_state() == sampler.get_rng_state()
    for e in (sampler, dev, user):
        e.close()


# ------------------------------------------------------------------ against float64
def _adam_rule(name, sizes, pname, got):
    """The first step's mu', nu', p' (target') of actor and critic by adam_ref's rule, on the engine's own gradient
    (probe engines fed the step's rows: a step from zero moments leaves mu' = (1 - b1) g)."""
    T, n, W, A, E = tc.SHAPES[name]
    cfg, st = _mid_state(name)
    batch, _, en, ec = _ref_run(name, sizes)[2][0][:4]
    ids, hp = _ids(), ar.Hyper()
    omb1 = float(np.float32(1) - np.float32(hp.b1))

    def probe(critic_state, clips):
        eng = _engine(cfg, n, PREC[pname], clips=clips)
        s = st.copy()
        if not critic_state:
            s.critic_opt = om.AdamState.zeros(st.critic.size, np.float64)
        s.actor_opt = om.AdamState.zeros(st.actor.size, np.float64)
        _load(eng, s)
        eng.update(batch, en, ec)
        out = {net: eng.get_params(ids[net][1]).astype(np.float64) / omb1 for net in ("actor", "critic", "alpha")}
        eng.close()
        return out

    a = probe(False, False)
    g_c, g_alpha = a["critic"], a["alpha"]
    g_a = probe(True, "critic")["actor"]  # through the UPDATED critic: the critic exactly as in the run
    fails = []
    for net, g, p0, opt, mx, tgt in (("critic", g_c, st.critic, st.critic_opt, cfg.critic_max_grad_norm, st.critic_target),
                                     ("actor", g_a, st.actor, st.actor_opt, cfg.actor_max_grad_norm, None)):
        ref, lo, S, c = ar.yardstick(p0, g, opt.mu, opt.nu, K0, hp, mx, tgt)
        for q in S:
            arr = got["target"] if q == "target" else got[net][("p", "mu", "nu").index(q)]
            r = ar.units(arr, getattr(ref, q), S[q])
            print(f"{name} {sizes} {pname} {net} {q}': engine {r:.2f} yardstick {c[q]:.2f} units")
            if not r <= 4 * c[q]:
                fails.append((net, q, r, c[q]))
    assert not fails, fails
    return g_c, g_a, g_alpha


@pytest.mark.parametrize("pname", list(PREC))
@pytest.mark.parametrize("name,sizes", tc.CASES, ids=tc.CASE_IDS)
def test_three_device_sampled_steps_match_float64(name, sizes, pname):
    T, n, W, A, E = tc.SHAPES[name]
    cfg, st_end, steps = _ref_run(name, sizes)
    _, st0 = _mid_state(name)
    ids = _ids()
    eng = _sampling_engine(name, sizes, pname, st0)
    eng.set_task_loss_logging(True)
    first = None
    for k, (batch, task, en, ec, want, internals) in enumerate(steps):
        eng.update(None, en, ec)
        _check_logs(eng.logs(), want, (name, sizes, pname, k))
        # per-task means of the per-row loss terms
        q, y = internals["q"][..., 0], internals["y"][:, 0]
        crit = ((q - y[None]) ** 2).mean(axis=0)
        act = internals["alpha_rows"][:, 0] * internals["logpi_cur"].reshape(-1) - internals["q_pi"].min(axis=0)[:, 0]
        tl = eng.task_losses()
        for t in range(T):
            rows = task == t
            assert rows.sum() == sizes[t]
            for w, term in enumerate((crit, act)):
                want_t = float(term[rows].mean()) if sizes[t] else 0.0
                print("task loss", k, t, w, tl[w, t], want_t)
                if sizes[t] == 0:
                    assert tl[w, t] == 0.0
                else:
                    assert abs(tl[w, t] - want_t) <= 1e-5 * abs(want_t), (name, sizes, pname, k, t, w, tl[w, t], want_t)
        if k == 0:
            first = {net: [eng.get_params(i) for i in ids[net]] for net in ("actor", "critic")}
            first["target"] = eng.get_params(ids["target"])
    _check_state(eng, st_end, len(steps), (name, sizes, pname))
    assert [eng.get_adam_count(i) for i in range(3)] == [K0 + 3, K0 + 3, 3]
    eng.close()
    g_c, g_a, g_alpha = _adam_rule(name, sizes, pname, first)
    # an empty task: its heads' gradients and its temperature gradient are exactly 0
    shapes = {"critic": om.critic_leaf_shapes(cfg), "actor": om.actor_leaf_shapes(cfg)}
    for t in range(T):
        hb_c, hW_c = (om.unflatten(g_c, shapes["critic"])[k][:, t] for k in ("head_b", "head_W"))
        hb_a, hW_a = (om.unflatten(g_a, shapes["actor"])[k][t] for k in ("head_b", "head_W"))
        if sizes[t] == 0:
            assert not hb_c.any() and not hW_c.any() and not hb_a.any() and not hW_a.any() and g_alpha[t] == 0.0, t
        else:
            assert hW_c.any() and hW_a.any() and g_alpha[t] != 0.0, t


# ------------------------------------------------------------------ step forms
def _run_form(name, pname, form, plan, logging=False):
    """plan: [(sizes or None, steps), ...] on one engine with device noise; form 'eager' issues single steps."""
    _, st = _mid_state(name)
    eng = _sampling_engine(name, None, pname, st)
    if form == "pipelined":
        eng.lib.mtsac_debug_set_pipeline(eng._h, 1)
    if logging:
        eng.set_task_loss_logging(True)
    eng.enable_graph(form == "graph")
    snaps = []
    for sizes, k in plan:
        eng.set_task_batch_sizes(None if sizes is None else np.array(sizes))
        if form == "eager":
            for _ in range(k):
                eng.update()
        else:
            eng.update_many(k)
        snaps.append(_snapshot(eng) + ([eng.task_losses()] if logging else []))
    state = eng.get_rng_state()
    eng.close()
    return snaps, state


PLANS = {
    "t3": [((9, 8, 7), 3), ((1, 0, 23), 2), (None, 1), ((24, 0, 0), 2)],
    "t4": [((7, 6, 4, 3), 2), ((0, 20, 0, 0), 3)],
    "t1": [((5,), 3)],
}


@pytest.mark.parametrize("pname", ["fp32", "split2h"])
@pytest.mark.parametrize("form", ["many", "graph", "pipelined"])
@pytest.mark.parametrize("name", list(PLANS))
def test_step_forms_agree_bitwise(name, form, pname):
    """update_many(k) (eager issue), hipGraph replay (the sizes change under a captured graph: the kernels read them
    from the device; setting and clearing the mode re-captures) and the pipelined lanes against single eager steps."""
    want, want_rng = _run_form(name, pname, "eager", PLANS[name])
    got, got_rng = _run_form(name, pname, form, PLANS[name])
    assert got_rng == want_rng
    for k, (a, b) in enumerate(zip(got, want)):
        _assert_same_bits(a, b, (name, form, pname, k))


def test_graph_is_enabled_in_uneven_mode_and_replays():
    """The graph decision: mtsac_enable_graph(1) succeeds with sizes set (the surgery modes refuse it)."""
    name = "t3"
    _, st = _mid_state(name)
    eng = _sampling_engine(name, (9, 8, 7), "fp32", st)
    eng.enable_graph(True)
    eng.update_many(2)
    assert eng.get_adam_count(1) == K0 + 2 and all(np.isfinite(v) for v in eng.logs().values())
    eng.close()


@pytest.mark.parametrize("pname", ["fp32", "split2h"])
def test_loss_logging_leaves_the_step_unchanged(pname):
    name = "t3"
    off, _ = _run_form(name, pname, "many", PLANS[name])
    on, _ = _run_form(name, pname, "many", PLANS[name], logging=True)
    for k, (a, b) in enumerate(zip(on, off)):
        _assert_same_bits(a[:len(b)], b, (pname, k))
    # the reduction follows the batch in force: zeros exactly where a task had no rows, balanced steps included
    for (sizes, _), snap in zip(PLANS[name], on):
        tl = snap[-1]
        empty = np.array([s == 0 for s in (sizes or (8, 8, 8))])
        assert np.all(tl[:, empty] == 0) and np.all(tl[0, ~empty] > 0) and np.all(np.isfinite(tl))
    # pipelined and graph steps reduce the same values
    for form in ("graph", "pipelined"):
        other, _ = _run_form(name, pname, form, PLANS[name], logging=True)
        for k, (a, b) in enumerate(zip(other, on)):
            _assert_same_bits(a, b, (pname, form, k))


def test_eval_passes_keep_sampling_interleaved_rows():
    """mtsac_task_gradients and mtsac_network_metrics with batch == NULL draw a balanced, interleaved sample while
    sizes are set (a task-major batch would fail their interleaved-rows check), and advance the stream as one
    balanced integers() call does."""
    name, sizes = "t3", (1, 0, 23)
    T, n, W, A, E = tc.SHAPES[name]
    _, st = _mid_state(name)
    eng = _sampling_engine(name, sizes, "fp32", st)
    rng = np.random.default_rng(SEED)
    eng.task_gradients()
    rng.integers(0, tc.CAPACITY, size=n)
    assert eng.get_rng_state() == rng.bit_generator.state
    assert eng.get_task_gradients(0).shape[0] == T and np.all(np.abs(eng.get_task_gradients(0)).sum(axis=1) > 0)
    eng.network_metrics()
    rng.integers(0, tc.CAPACITY, size=n)
    assert eng.get_rng_state() == rng.bit_generator.state
    assert eng.task_batch_sizes().tolist() == list(sizes)
    _, rows = eng.sample()  # the step's own sampling is still uneven
    np.testing.assert_array_equal(np.argmax(rows[0][:, 39:], axis=1), np.repeat(np.arange(T), sizes))
    eng.close()
