"""The SAC optimizer step (optim.hip: clip / Adam / Polyak / temperature) element by element against
float64 from mid-training states, and the derived weight copies it writes for the next step's GEMMs.

The gradient every check feeds the reference is the engine's own, read back from probe runs (a step
from zero moments leaves mu' = (1 - b1) g), so the same assertions hold at every GEMM precision.
Allowances come from adam_ref: 4 times the error of the numpy float32 evaluation of the same formulas
on the same inputs, in units of 2^-24 times each formula's absolute terms (adam_ref.scales).

Measured on one MI355X, worst over every run of a test: the engine's error in units of 2^-24 S, the
numpy float32 yardstick's on the same inputs, and the largest engine / yardstick ratio of any single
run (the allowance is 4; every test prints its own figures):

    quantity                 engine   yardstick   worst ratio
    actor / critic mu'       1.86     1.71        1.23
    actor / critic nu'       1.93     1.97        1.27
    actor / critic p'        0.99     0.99        1.00
    target'                  2.00     2.06        1.00
    log_alpha mu', nu', p'   1.50     1.50        2.00   (nu' at 0.99 of a unit against the 0.5 floor)
    grad magnitudes (rel)    1.0e-7   1.5e-7      1.67
    params norms (rel)       9.5e-8   9.5e-8      1.29
    alpha log (rel)          6.9e-8   9.7e-8      1.16

The temperature gradient is within 0.014 of its allowance against the oracle; a plain-step gradient
element at most 1.3e-6 mag (1e-5 allowed), and up to 9.8e-2 of the plain product |in|^T |dz|, which
grad_mag_ref explains is not a bound (the float32 oracle misses 1e-5 of it too).
"""

from __future__ import annotations

import math

import numpy as np
import pytest

import adam_ref as ar
import grad_mag_ref as gm
import sac_opt_cases as sc
from oracle import mtsac as om

pytestmark = pytest.mark.gpu

NETS = ("actor", "critic", "alpha")
LOSS_RTOL = 1e-5  # the suite's bar for losses against the oracle (test_gpu_update.py)


def _tensor_ids():
    from mtrl_amd import _lib as L

    return {"actor": (L.ACTOR, L.ACTOR_ADAM_MU, L.ACTOR_ADAM_NU), "critic": (L.CRITIC, L.CRITIC_ADAM_MU, L.CRITIC_ADAM_NU),
            "alpha": (L.LOG_ALPHA, L.ALPHA_ADAM_MU, L.ALPHA_ADAM_NU), "target": (L.CRITIC_TARGET,)}


def _engine(cfg: om.OracleConfig, n: int, hs: sc.HyperSet, clips, precision: int):
    from mtrl_amd.engine import MTSACEngine, make_config

    c = make_config(
        precision=precision, num_tasks=cfg.num_tasks, task_count=sc.owned_tasks(cfg.num_tasks), obs_dim=cfg.obs_dim,
        action_dim=cfg.action_dim, actor_width=cfg.actor_width, actor_depth=cfg.actor_depth,
        critic_width=cfg.critic_width, critic_depth=cfg.critic_depth, num_critics=cfg.num_critics, batch_per_task=n,
        capacity=64, gamma=cfg.gamma, tau=hs.tau, clip=int(cfg.clip), use_task_weights=int(cfg.use_task_weights),
        actor_lr=hs.actor_lr, critic_lr=hs.critic_lr, alpha_lr=hs.alpha_lr, adam_b1=hs.b1, adam_b2=hs.b2,
        adam_eps=hs.eps, actor_max_grad_norm=clips[0], critic_max_grad_norm=clips[1], alpha_max_grad_norm=clips[2])
    e = MTSACEngine(c)
    e.enable_graph(False)
    return e


def _read(eng) -> dict:
    """All ten tensors, the three counts and the logs."""
    ids = _tensor_ids()
    out = {"logs": eng.logs(), "counts": tuple(eng.get_adam_count(i) for i in range(3))}
    for net in NETS:
        out[net] = dict(zip(("p", "mu", "nu"), (eng.get_params(i) for i in ids[net])))
    out["critic"]["target"] = eng.get_params(ids["target"][0])
    return out


def _load(eng, params: dict, moments: dict, counts):
    """params: actor, critic, target, alpha; moments: {net: (mu, nu)} (a missing net keeps its zeros)."""
    ids = _tensor_ids()
    for net in NETS:
        eng.set_params(ids[net][0], params[net])
        if net in moments:
            eng.set_params(ids[net][1], moments[net][0])
            eng.set_params(ids[net][2], moments[net][1])
    eng.set_params(ids["target"][0], params["target"])
    for i in range(3):
        eng.set_adam_count(i, counts[i])


def _base_params(name, T=None) -> dict:
    st = sc.base_state(name, T)[0]
    cfg = sc.oracle_config(name, T)
    return {"actor": sc.local_flat(cfg, st.actor, "actor"), "critic": sc.local_flat(cfg, st.critic, "critic"),
            "target": sc.local_flat(cfg, st.critic_target, "critic"), "alpha": st.log_alpha}


def _run(name, T, precision, hs, clips, moments, counts, clip_tw=False):
    """One step of a fresh engine from the base state with the given optimizer state; (_read, forms)."""
    cfg = sc.oracle_config(name, T, clip=clip_tw, use_task_weights=clip_tw)
    batch, en, ec = sc.local_rows(cfg, *sc.base_state(name, T)[1:4])
    eng = _engine(cfg, sc.rows_per_task(name), hs, clips, precision)
    _load(eng, _base_params(name, T), moments, counts)
    eng.update(batch, en, ec)
    out = _read(eng)
    forms = (eng.opt_form(0), eng.opt_form(1))
    eng.close()
    return out, forms


def _grad_from_probe(mu_new, b1: float) -> np.ndarray:
    """g of a step from zero moments: the engine stored mu' = fl((1 - b1) g) with 1 - b1 in float32."""
    omb1 = float(np.float32(1) - np.float32(b1))
    return np.asarray(mu_new, np.float64) / omb1


def _probes(name, T, precision, hs, clips, moments):
    """{net: unclipped gradient of the run under test}.  Probe A (everything from zero, no clip): the
    critic's and the temperature's, which depend on no optimizer state.  Probe B (the critic exactly as
    in the run, the actor from zero without clip): the actor's, which is differentiated through the
    updated critic."""
    zero_hs = sc.HyperSet(**{**hs.__dict__, "counts": (0, 0, 0)})
    a, _ = _run(name, T, precision, zero_hs, (None, None, None), {}, (0, 0, 0))
    b, _ = _run(name, T, precision, hs, (None, clips[1], None), {"critic": moments["critic"]},
                (0, hs.counts[1], 0))
    b1 = ar.f32(hs.b1)
    return {"critic": _grad_from_probe(a["critic"]["mu"], b1), "alpha": _grad_from_probe(a["alpha"]["mu"], b1),
            "actor": _grad_from_probe(b["actor"]["mu"], b1)}, a, b


def _scalar(report, fails, tag, got, ref, lo):
    """A scalar log, relative: 4 times the float32 yardstick's error, which for one number is at least
    its own rounding to float32 (2^-24)."""
    yard = max(abs(float(lo) - ref) / abs(ref), ar.U24)
    err = abs(got - ref) / abs(ref)
    report.append(f"{tag}: engine {err:.2e} yardstick {yard:.2e} ratio {err / yard:.2f}")
    if not err <= 4 * yard:
        fails.append((tag, got, ref, err, yard))
    return err / yard


def _check_net(report, fails, tag, got: dict, p0, g, mom, k0, hp, mx, target0=None):
    """mu', nu', p' (target') of one network against adam_ref; returns (ref, lo)."""
    mu0, nu0 = (np.asarray(x, np.float64) for x in mom)
    ref, lo, S, c = ar.yardstick(p0, g, mu0, nu0, k0, hp, mx, target0)
    for q in S:
        r = ar.units(got[q], getattr(ref, q), S[q])
        report.append(f"{tag} {q}': engine {r:.2f} yardstick {c[q]:.2f} units, ratio {r / c[q]:.2f}")
        if not r <= 4 * c[q]:
            fails.append((tag, q, r, c[q]))
    return ref, lo


def _check_run(name, T, precision, hs, clips):
    """Probes + run R + every assertion of part 1; returns (R, probe A, gradients, forms)."""
    moments = sc.start_moments(name, hs, T)
    g, probe_a, _ = _probes(name, T, precision, hs, clips, moments)
    R, forms = _run(name, T, precision, hs, clips, moments, hs.counts)
    P = _base_params(name, T)
    report, fails = [], []
    refs = {}
    for i, net in enumerate(NETS):
        refs[net] = _check_net(report, fails, net, R[net], P[net], g[net], moments[net], hs.counts[i], hs.hyper(net),
                               clips[i], P["target"] if net == "critic" else None)
        if clips[i] is not None:  # the threshold sits where the case wants it
            assert refs[net][0].clipped == (clips[i] < refs[net][0].gnorm) and \
                not 0.5 * clips[i] < refs[net][0].gnorm < 2 * clips[i], (net, clips[i], refs[net][0].gnorm)
    if R["counts"] != tuple(k + 1 for k in hs.counts):
        fails.append(("counts", R["counts"]))
    logs = R["logs"]
    for net in ("critic", "actor"):
        ref, lo = refs[net]
        _scalar(report, fails, f"{net}_grad_magnitude", logs[f"metrics/{net}_grad_magnitude"], ref.gnorm,
                ar.global_norm(g[net], np.float32))
        _scalar(report, fails, f"{net}_params_norm", logs[f"metrics/{net}_params_norm"], float(ar.global_norm(ref.p)),
                ar.global_norm(lo.p, np.float32))
    ref, lo = refs["alpha"]
    _scalar(report, fails, "alpha", logs["alpha"], float(np.sum(np.exp(ref.p))), np.sum(np.exp(lo.p), dtype=np.float32))
    print("\n".join(report))
    assert not fails, fails
    return R, probe_a, g, forms, refs


# ---------------------------------------------------------------------------- forms
def _expected_form(name, precision):
    """opt_params (engine.cpp): fp32 has no planes; a trunk with hidden kernels at these sizes is a
    gemm_x3f / gemm_x3s net (tiles_fusable); the one-layer trunk is not (x3f needs depth > 1) and its
    planes have the leaf's layout (planes_fusable: width 64 = its padded leading dimension)."""
    return 0 if precision == 0 else 1 if sc.CASES[name]["depth"] == 1 else 2


def test_every_optimizer_form_occurs():
    """Elementwise, plane segments, tiles and the transposed head write are all taken somewhere in the
    parametrisation below (mtsac_debug_opt_form answers through optimize()'s own predicates)."""
    seen, wht = set(), False
    for name in sc.CASES:
        for pname, precision in sc.PRECISIONS.items():
            cfg = sc.oracle_config(name)
            eng = _engine(cfg, sc.rows_per_task(name), sc.HyperSet(), (None, None, None), precision)
            fa, fc = eng.opt_form(0), eng.opt_form(1)
            eng.close()
            print(name, pname, "actor", fa, "critic", fc)
            assert fa & 3 == fc & 3 == _expected_form(name, precision), (name, pname, fa, fc)
            assert not (fa | fc) & 32 and not fc & 16  # nothing sharded; only the actor has a transposed head
            seen |= {fa & 3, fc & 3}
            wht |= bool(fa & 16)
    assert seen == {0, 1, 2} and wht
    with pytest.raises(Exception):
        eng = _engine(sc.oracle_config("tiny"), 4, sc.HyperSet(), (None, None, None), 0)
        try:
            eng.opt_form(2)
        finally:
            eng.close()


# ---------------------------------------------------------------------------- part 1
RUNS = [(name, "b", "none") for name in sc.CASES] + \
       [(name, hset, "none") for name in sc.SMALL for hset in ("a", "c")] + \
       [(name, "b", clip) for name in sc.SMALL for clip in ("quarter", "four", "zero")]


@pytest.mark.parametrize("pname", list(sc.PRECISIONS))
@pytest.mark.parametrize("name,hset,clip", RUNS, ids=["-".join(r) for r in RUNS])
def test_optimizer_step_matches_float64(name, hset, clip, pname):
    """Run R of the issue: generated moments, the set's counts, clips and hyper-parameters, one step;
    mu', nu', p', target' of actor, critic and temperature elementwise, the counts and the five logs the
    optimizer produces.  Set (a) starts at count 0, which only zero moments reach."""
    hs = sc.hyper_set(name, hset)
    clips = sc.clip_thresholds(name, clip)
    R, _, g, forms, refs = _check_run(name, None, sc.PRECISIONS[pname], hs, clips)
    assert forms[0] & 3 == forms[1] & 3 == _expected_form(name, sc.PRECISIONS[pname])
    # the probes' gradient reaches every leaf (w64_d1 under the plane precisions once left dW_0 = 0: a
    # self-consistent optimizer check cannot see a gradient that is missing on both of its sides)
    cfg = sc.oracle_config(name)
    for net, shapes in (("critic", om.critic_leaf_shapes(cfg)), ("actor", om.actor_leaf_shapes(cfg))):
        for leaf, v in om.unflatten(g[net], shapes).items():
            assert np.count_nonzero(v) > v.size // 2, (net, leaf, int(np.count_nonzero(v)), v.size)
    if clip == "zero":  # the gradient is gone, the old momentum still moves the parameters
        for net in ("actor", "critic"):
            mu0, nu0 = sc.start_moments(name, hs)[net]
            np.testing.assert_array_equal(R[net]["mu"], np.float32(hs.b1) * mu0)
            np.testing.assert_array_equal(R[net]["nu"], np.float32(hs.b2) * nu0)
            assert np.any(R[net]["p"] != _base_params(name)[net].astype(np.float32))


# ---------------------------------------------------------------------------- part 2
@pytest.mark.parametrize("pname", ["fp32", "split2h"])
@pytest.mark.parametrize("clip", ["none", "quarter", "four"])
@pytest.mark.parametrize("T", [3, 33, 64, 65, 67])
def test_temperature_optimizer_both_paths(T, clip, pname):
    """alpha_adam_wave's one-task-a-lane path (T <= 64) and its strided loop (65, 67), alpha_tasks past
    its 32-task stride (33): log_alpha', its moments and the alpha log from generated moments at count
    7, with and without alpha_max_grad_norm; the gradient and the loss against the oracle.  An engine
    owns at most 64 tasks, so 65 and 67 run as the task shard that owns tasks [0, 64): log_alpha and its
    moments keep all T entries and Adam steps every one of them (the other shards' with a zero gradient,
    by their old momentum), which is the T_glob > 64 loop."""
    name = "alpha"
    hs = sc.HyperSet(counts=(7, 7, 7))
    ca = sc.clip_thresholds(name, clip, T)[2]
    R, probe_a, g, _, _ = _check_run(name, T, sc.PRECISIONS[pname], hs, (None, None, ca))
    o = sc.oracle_pass(name, T)
    batch = sc.base_state(name, T)[1]
    task = np.argmax(batch[0][:, -T:], axis=1)
    B = task.size
    lp = o["logpi_cur"].reshape(-1) + o["cfg"].target_entropy
    allow = 1e-5 * np.bincount(task, weights=np.abs(lp), minlength=T) / B
    # a shard (T > 64: tasks [0, 64) of T) computes its own tasks' part of the global gradient and loss,
    # normalised by the global row count; the tasks of other shards get exactly 0 until the all-reduce
    tc = sc.owned_tasks(T)
    want_g = np.where(np.arange(T) < tc, o["alpha_grad"], 0.0)
    d = np.abs(g["alpha"] - want_g)
    print("alpha grad: worst error / allowance", float(np.max(d[:tc] / allow[:tc])))
    assert np.all(d[:tc] <= allow[:tc]) and np.all(g["alpha"][tc:] == 0), (d / allow)
    st = sc.base_state(name, T)[0]
    want = float(np.sum((-st.log_alpha[task] * lp)[task < tc]) / B)
    if tc == T:
        assert abs(want - o["logs"]["losses/alpha_loss"]) <= 1e-12 * abs(want)
    for logs in (probe_a["logs"], R["logs"]):  # the loss uses log_alpha before the step
        assert abs(logs["losses/alpha_loss"] - want) <= LOSS_RTOL * abs(want), (logs["losses/alpha_loss"], want)


# ---------------------------------------------------------------------------- part 3
def _plane_exp(bound: float) -> int:
    """gemm_common.h plane_exp on the host."""
    b = float(np.float32(np.float32(bound) * np.float32(1.00390625)))
    if not (b > 0.0 and b < 3.0e38):
        return 0
    return min(100, max(-100, 15 - math.frexp(b)[1]))


def _trunk_max(cfg, flat, critic: bool) -> float:
    """max |.| over the trunk leaves (everything after the two head leaves in flat order)."""
    shapes = om.critic_leaf_shapes(cfg) if critic else om.actor_leaf_shapes(cfg)
    heads = sum(int(np.prod(s)) for _, s in shapes[:2])
    return float(np.max(np.abs(flat[heads:])))


def _assert_same_plane_exponents(name, cfg, hs, before, after):
    """split2h: continuing, the planes step 2 reads carry plane_exp(max |p| before step 1 + w_add)
    (optim.hip h2_scales; the target: the larger of that and max |target| before); reloaded, the
    exponent of the exact maximum after step 1 (weights_record_kernel).  The inputs are chosen so that
    both are the same power of two: the whole interval max |p| -+ w_add, which contains the maximum after
    any step, lies in one binade."""
    r = max(1.0, max(math.sqrt(1 - hs.b2 ** t) / (1 - hs.b1 ** t) for t in range(1, 2000)))
    bound = 1.25 * r * ar.moment_ratio_bound(ar.f32(hs.b1), ar.f32(hs.b2))  # engine.cpp adam_step_bound_of
    for net, critic in (("actor", False), ("critic", True)):
        w_add = bound * getattr(hs, net + "_lr")
        m0 = _trunk_max(cfg, before[net], critic)
        m1 = _trunk_max(cfg, after[net]["p"], critic)
        e = _plane_exp(m0 + w_add)
        print(f"{name} {net}: trunk max {m0:.6f} -> {m1:.6f}, w_add {w_add:.2e}, exponent {e}, "
              f"binade margin {min(m0 * 1.00390625 / 2.0 ** (14 - e), 2.0 ** (15 - e) / (m0 * 1.00390625)):.3f}")
        assert _plane_exp(m0 - w_add) == e == _plane_exp(m1), (net, m0, m1, w_add)
        if critic:
            t0 = _trunk_max(cfg, before["target"], True)
            t1 = _trunk_max(cfg, after[net]["target"], True)
            assert _plane_exp(max(t0, m0 + w_add)) == _plane_exp(t1), (t0, t1)


@pytest.mark.parametrize("pname", list(sc.PRECISIONS))
@pytest.mark.parametrize("name", list(sc.CASES))
def test_continue_equals_reload(name, pname):
    """Engine X runs two steps; engine Y is loaded through set_params with X's ten tensors and three
    counts after the first and runs the second.  X reads in step 2 what its optimizer wrote (tiles,
    plane segments, the transposed head), Y what split_planes, head_transpose and weights_record built
    from the same values: all ten tensors and the ten logs are bitwise equal afterwards."""
    precision = sc.PRECISIONS[pname]
    hs = sc.HyperSet(counts=(9, 9, 9))
    clips = (1.0, 1.0, None)  # the engine's defaults
    cfg = sc.oracle_config(name)
    n = sc.rows_per_task(name)
    st, b1, en1, ec1, b2, en2, ec2 = sc.base_state(name)
    moments = sc.start_moments(name, hs)
    P = _base_params(name)
    X = _engine(cfg, n, hs, clips, precision)
    _load(X, P, moments, hs.counts)
    X.update(b1, en1, ec1)
    mid = _read(X)
    if pname == "split2h":
        _assert_same_plane_exponents(name, cfg, hs, P, mid)
    X.update(b2, en2, ec2)
    x = _read(X)
    X.close()
    Y = _engine(cfg, n, hs, clips, precision)
    _load(Y, {"actor": mid["actor"]["p"], "critic": mid["critic"]["p"], "target": mid["critic"]["target"],
              "alpha": mid["alpha"]["p"]}, {net: (mid[net]["mu"], mid[net]["nu"]) for net in NETS}, mid["counts"])
    Y.update(b2, en2, ec2)
    y = _read(Y)
    Y.close()
    assert x["counts"] == y["counts"] == (11, 11, 11)
    bad = [(net, q, int(np.sum(x[net][q] != y[net][q])), float(np.max(np.abs(x[net][q] - y[net][q]))))
           for net in NETS for q in x[net] if not np.array_equal(x[net][q], y[net][q])]
    bad += [(k, x["logs"][k], y["logs"][k]) for k in x["logs"] if x["logs"][k] != y["logs"][k]]
    assert not bad, bad


# ---------------------------------------------------------------------------- part 4
GRAD_CASES = [(name, False) for name in sc.CASES] + [("tiny", True)]


@pytest.mark.parametrize("pname", ["fp32", "split3", "split2h"])
@pytest.mark.parametrize("name,clip_tw", GRAD_CASES, ids=[n + ("-clip_tw" if c else "") for n, c in GRAD_CASES])
def test_plain_step_gradients_leaf_by_leaf(name, clip_tw, pname):
    """The plain step's gradients (a step from zero moments without clips: mu' / (1 - b1)) against the
    float64 oracle, every element of every leaf within 1e-5 mag (grad_mag_ref)."""
    hs = sc.HyperSet()
    out, _ = _run(name, None, sc.PRECISIONS[pname], hs, (None, None, None), {}, (0, 0, 0), clip_tw=clip_tw)
    o = sc.oracle_pass(name, clip_tw=clip_tw)
    cfg = o["cfg"]
    fails = []
    for net, shapes in (("critic", om.critic_leaf_shapes(cfg)), ("actor", om.actor_leaf_shapes(cfg))):
        g = _grad_from_probe(out[net]["mu"], ar.f32(hs.b1))
        plain = dict((leaf, w) for leaf, w, _ in gm.leaf_report(g, o[net + "_grad"], o["plain_" + net], shapes))
        for leaf, worst, exact in gm.leaf_report(g, o[net + "_grad"], o["mag_" + net], shapes):
            print(f"{net} {leaf}: worst error / mag {worst:.2e} (/ plain product {plain[leaf]:.2e}), zeros exact {exact}")
            if not (exact and worst <= gm.GRAD_RTOL):
                fails.append((net, leaf, worst, exact))
    assert not fails, fails
