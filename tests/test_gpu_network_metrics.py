"""The network health metrics on the device: the two kernels alone (mtsac_debug_act_stats / _act_gram) at edge
shapes, the whole pass against the float64 oracle forward with propagated bars, no side effects on training,
and the compat layer's get_metrics.  Statements and bars: tests/network_metrics_ref.py."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import network_metrics_ref as R

pytestmark = pytest.mark.gpu

# (Z, M, W, ld): both Gram sides, W and M off the MFMA tile's 16 and 4, ld > W, more than one 64 x 64 tile
KERNEL_SHAPES = [(1, 1, 4, 4), (1, 64, 16, 16), (2, 3, 20, 20), (1, 15, 36, 40), (3, 130, 132, 132), (2, 257, 516, 516)]
U24 = 2.0 ** -24


def _lib():
    from mtrl_amd import _lib as L

    return L, L.load()


def _padded(H, ld):
    """[Z][M][ld] float32 with NaN in the padding columns."""
    Z, M, W = H.shape
    out = np.full((Z, M, ld), np.nan, np.float32)
    out[:, :, :W] = H
    return out


def act_stats(H, ld, threshold=0.1):
    L, lib = _lib()
    Z, M, W = H.shape
    Hp = _padded(H, ld)
    score, norm = np.empty((Z, W), np.float32), np.empty((Z, W), np.float32)
    count = np.empty(Z, np.int32)
    L.check(lib.mtsac_debug_act_stats(Z, M, W, ld, Hp.ctypes.data, ctypes.c_float(threshold), score.ctypes.data,
                                      norm.ctypes.data, count.ctypes.data))
    return score, norm, count


def act_gram(H, ld):
    L, lib = _lib()
    Z, M, W = H.shape
    r = min(M, W)
    Hp = _padded(H, ld)
    G = np.empty((Z, r, r), np.float64)
    info = np.full(2, -1, np.int32)
    L.check(lib.mtsac_debug_act_gram(Z, M, W, ld, Hp.ctypes.data, G.ctypes.data, info.ctypes.data))
    assert info[0] == (0 if W <= M else 1) and info[1] == r
    return G


def _relu_data(Z, M, W, seed):
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((Z, M, W)) + 0.3, 0).astype(np.float32)


# ------------------------------------------------------------------ Gram kernel
@pytest.mark.parametrize("Z,M,W,ld", KERNEL_SHAPES)
def test_gram_exact_on_small_integers(Z, M, W, ld):
    """Small integers: every product and partial sum is exact in fp64, so the result equals the integer
    computation bit for bit.  Columns and rows are distinct and the matrix has no symmetry, so an output
    written at another lane's (row, col) shows."""
    rng = np.random.default_rng(Z * 1000 + M + W)
    H = rng.integers(0, 8, (Z, M, W)).astype(np.int64)
    H += (np.arange(W)[None, None, :] % 5) + 2 * (np.arange(M)[None, :, None] % 3)
    G = act_gram(H.astype(np.float32), ld)
    for z in range(Z):
        want = H[z].T @ H[z] if W <= M else H[z] @ H[z].T
        assert len({tuple(c) for c in want.tolist()}) == want.shape[0]  # distinct rows: a permutation shows
        assert np.array_equal(G[z], want.astype(np.float64)), (z, np.argwhere(G[z] != want)[:4])


@pytest.mark.parametrize("Z,M,W,ld", KERNEL_SHAPES)
def test_gram_bound_symmetry_determinism(Z, M, W, ld):
    """Random fp32 data: the products are exact in fp64, so |G - G64| <= M 2^-52 (|H|^T |H|) elementwise (the
    fp64 summation bound); G is bitwise symmetric and bitwise equal run to run."""
    rng = np.random.default_rng(7 * M + W)
    H = rng.standard_normal((Z, M, W)).astype(np.float32)
    G, G2 = act_gram(H, ld), act_gram(H, ld)
    assert G.tobytes() == G2.tobytes()
    worst = 0.0
    for z in range(Z):
        H64 = H[z].astype(np.float64)
        want, side = R.gram64(H64)
        S = np.abs(H64).T @ np.abs(H64) if side == 0 else np.abs(H64) @ np.abs(H64).T
        assert np.array_equal(G[z], G[z].T)
        bound = M * 2.0 ** -52 * S
        worst = max(worst, float(np.max(np.abs(G[z] - want) / bound)))
        assert np.all(np.abs(G[z] - want) <= bound), (z, worst)
    print(f"gram {Z, M, W, ld}: max |G - G64| / bound = {worst:.3g}")


# ------------------------------------------------------------------ statistics kernel
@pytest.mark.parametrize("Z,M,W,ld", KERNEL_SHAPES)
def test_scores_against_float64(Z, M, W, ld):
    """s and s~ within 4 * 2^-24 relative: the fp64 accumulation is negligible; what remains is one fp32
    rounding of s, one of the denominator and one of the quotient."""
    H = _relu_data(Z, M, W, 11 * M + W)
    score, norm, count = act_stats(H, ld)
    score2, norm2, count2 = act_stats(H, ld)
    assert score.tobytes() == score2.tobytes() and norm.tobytes() == norm2.tobytes() and np.array_equal(count, count2)
    for z in range(Z):
        s, sn = R.scores(H[z])
        assert np.all(np.abs(score[z] - s) <= 4 * U24 * np.abs(s))
        assert np.all(np.abs(norm[z] - sn) <= 4 * U24 * np.abs(sn))


@pytest.mark.parametrize("Z,M,W,ld", KERNEL_SHAPES)
def test_counts_on_planted_columns(Z, M, W, ld):
    """Dead columns (exactly zero), weak columns (scaled 0.02) and normal ones: no s~ within 1e-3 of 0.1, so
    the count is exact.  Negative entries check the absolute value."""
    rng = np.random.default_rng(13 * M + W)
    H = rng.uniform(0.9, 1.1, (Z, M, W)) * rng.choice([-1.0, 1.0], (Z, M, W))
    want = np.zeros(Z, int)
    for z in range(Z):
        kind = rng.integers(0, 3, W)  # 0 dead, 1 weak, 2 normal; at least half normal, so weak / mean < 0.05
        kind[: (W + 1) // 2] = 2
        kind = rng.permutation(kind)
        H[z][:, kind == 0] = 0.0
        H[z][:, kind == 1] *= 0.02
        want[z] = int(np.sum(kind < 2))
    H = H.astype(np.float32)
    for z in range(Z):
        sn = R.scores(H[z])[1]
        assert np.all(np.abs(sn - 0.1) > 1e-3) and R.dormant_count(H[z]) == want[z]
    _, _, count = act_stats(H, ld)
    assert np.array_equal(count, want)


@pytest.mark.parametrize("Z,M,W,ld", KERNEL_SHAPES)
def test_all_zero_matrix(Z, M, W, ld):
    H = np.zeros((Z, M, W), np.float32)
    score, norm, count = act_stats(H, ld)
    assert np.all(count == W) and np.all(score == 0) and np.all(norm == 0)
    assert np.all(act_gram(H, ld) == 0)


def test_debug_entries_refuse_bad_arguments():
    _, lib = _lib()
    x = np.zeros(16, np.float32)
    o = np.zeros(16, np.float64)
    i = np.zeros(4, np.int32)
    assert lib.mtsac_debug_act_gram(1, 2, 4, 3, x.ctypes.data, o.ctypes.data, i.ctypes.data) == -22  # ld < W
    assert lib.mtsac_debug_act_stats(1, 2, 4, 4, x.ctypes.data, ctypes.c_float(np.nan), o.ctypes.data, x.ctypes.data,
                                     i.ctypes.data) == -22


# ------------------------------------------------------------------ whole path
PRECISIONS = ["split2h", "split3", "fp32"]


@functools.lru_cache(maxsize=None)
def _expect(shape):
    seed, protos = R.WHOLE_CASES[shape]
    return R.case_expectations(shape, seed, protos)


def _engine(shape, precision, actor, critic, **kw):
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config

    T, n, W, D, A, E = shape
    eng = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, action_dim=A, actor_width=W, actor_depth=D,
                                  critic_width=W, critic_depth=D, num_critics=E, batch_per_task=n, capacity=64,
                                  precision=L.PRECISIONS[precision], **kw))
    eng.set_params(L.ACTOR, actor)
    eng.set_params(L.CRITIC, critic)
    eng.set_params(L.CRITIC_TARGET, critic)
    return eng


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", list(R.WHOLE_CASES))
def test_whole_path_against_oracle(shape, precision):
    """Scores within the bar propagated from the documented GEMM bound through the float64 forward; counts and
    srank exact.  The margin conditions on the inputs are asserted on the reference alone first."""
    from mtrl_amd import netmetrics as NM

    (cfg, actor, critic, obs, eps), exp, ok = _expect(shape)
    assert ok, "the float64 reference must keep its margins from 0.1 and from 0.99 (tests/network_metrics_ref.py)"
    T, n, W, D, A, E = shape
    eng = _engine(shape, precision, actor, critic)
    try:
        out = eng.network_metrics(obs, eps)
    finally:
        eng.close()
    assert set(exp) == set(NM.member_names(E))
    worst = 0.0
    for name, rows in exp.items():
        r = out["actor"] if name == "actor" else out["critic"]
        e = 0 if name == "actor" else int(name.split("_")[1])
        assert r["gram"][e][0].shape == (min(n * T, W),) * 2
        for i, want in enumerate(rows):
            got = r["scores"][e][i].astype(np.float64)
            err = np.abs(got - want["norm"])
            live = want["bar"] > 0  # a certainly dead neuron has bar 0: its score must be exactly 0
            worst = max(worst, float(np.max(err[live] / want["bar"][live])))
            assert np.all(err <= want["bar"]), (name, i, worst)
            assert int(r["counts"][e][i]) == want["count"], (name, i)
            assert NM.srank_from_gram(r["gram"][e][i]) == want["srank"], (name, i)
    print(f"whole path {shape} {precision}: max |s~ - ref| / bar = {worst:.3g}")


def test_whole_path_parts_and_device_inputs():
    """what = 1 / 2 alone give the same results as both together; a device-sampled batch with device noise runs
    and is deterministic for equal index and noise streams; bad arguments are refused."""
    from mtrl_amd._lib import MTSACError, check

    shape = (3, 5, 36, 3, 4, 2)
    (cfg, actor, critic, obs, eps), _, _ = _expect(shape)
    eng = _engine(shape, "split2h", actor, critic)
    try:
        both = eng.network_metrics(obs, eps)
        only_d = eng.network_metrics(obs, eps, dormant=True, gram=False)
        only_g = eng.network_metrics(obs, eps, dormant=False, gram=True)
        for net in ("actor", "critic"):
            assert only_d[net]["gram"] is None and only_g[net]["scores"] is None
            assert only_d[net]["scores"].tobytes() == both[net]["scores"].tobytes()
            assert np.array_equal(only_d[net]["counts"], both[net]["counts"])
            for a, b in zip(only_g[net]["gram"], both[net]["gram"]):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        with pytest.raises(MTSACError):  # the last call had no statistics
            check(eng.lib.mtsac_get_network_scores(eng._h, 0, None, None))
        with pytest.raises(MTSACError):
            eng.network_metrics(obs, eps, dormant=False, gram=False)
        with pytest.raises(MTSACError):
            eng.network_metrics(obs, eps, threshold=float("nan"))
        eng.buffer_fill_synthetic(3)
        runs = []
        for _ in range(2):
            eng.seed_rng(5)
            runs.append(eng.network_metrics(None, None))
        for net in ("actor", "critic"):
            assert runs[0][net]["scores"].tobytes() == runs[1][net]["scores"].tobytes()
            assert np.all(np.isfinite(runs[0][net]["scores"]))
    finally:
        eng.close()


# ------------------------------------------------------------------ no side effects
def _state(eng):
    return [eng.get_params(w).tobytes() for w in range(10)] + [eng.get_adam_count(i) for i in range(3)] + \
        [np.array(list(eng.logs().values()), np.float32).tobytes(), eng.noise_state()]


@pytest.mark.parametrize("mode", ["eager", "graph", "pcgrad"])
def test_no_side_effects_between_updates(mode):
    """Two engines from one state; one calls network_metrics (injected batch and eps) between two updates:
    parameters, Adam moments, counts, logs and the noise stream stay bitwise equal."""
    from helpers import synthetic_batch, synthetic_eps

    shape = (3, 5, 36, 3, 4, 2)
    T, n, W, D, A, E = shape
    (cfg, actor, critic, obs, eps), _, _ = _expect(shape)
    engines = [_engine(shape, "split2h", actor, critic, noise_seed=9) for _ in range(2)]
    try:
        states = []
        for k, eng in enumerate(engines):
            if mode == "pcgrad":
                eng.set_pcgrad(True)
            if mode == "graph":
                eng.buffer_fill_synthetic(3)
                eng.seed_rng(5)
                eng.enable_graph(True)
                eng.update_many(2)
            else:
                b1 = synthetic_batch(T, n * T, action_dim=A, seed=1, dtype=np.float32)
                eng.update(b1, *synthetic_eps(n * T, action_dim=A, seed=2, dtype=np.float32))
            if k == 1:
                out = eng.network_metrics(obs, eps)
                assert np.all(np.isfinite(out["critic"]["scores"]))
            if mode == "graph":
                eng.update_many(2)
            else:
                b2 = synthetic_batch(T, n * T, action_dim=A, seed=3, dtype=np.float32)
                eng.update(b2, *synthetic_eps(n * T, action_dim=A, seed=4, dtype=np.float32))
            states.append(_state(eng))
        assert states[0] == states[1]
    finally:
        for eng in engines:
            eng.close()


def test_sharded_engine_refuses():
    from mtrl_amd._lib import MTSACError
    from mtrl_amd.engine import MTSACEngine, make_config

    e = MTSACEngine(make_config(num_tasks=4, task_begin=2, task_count=2, obs_dim=43, actor_width=32, critic_width=32,
                                batch_per_task=4, capacity=64, precision=1))
    try:
        with pytest.raises(MTSACError, match="-95"):
            e.network_metrics()
    finally:
        e.close()


# ------------------------------------------------------------------ compat layer
def _experiment(tmp_path, T, total=600):
    from fake_env import FakeMetaworldConfig
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.config.rl import OffPolicyTrainingConfig
    from mtrl.experiment import Experiment
    from mtrl.rl.algorithms import MTSACConfig

    return Experiment(
        exp_name="fake_metrics", seed=1, data_dir=tmp_path, env=FakeMetaworldConfig(env_id="MT10"),
        algorithm=MTSACConfig(
            num_tasks=T, gamma=0.99,
            actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(
                num_tasks=T, width=64, optimizer=OptimizerConfig(max_grad_norm=1.0))),
            critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(
                num_tasks=T, width=64, optimizer=OptimizerConfig(max_grad_norm=1.0))),
            num_critics=2),
        training_config=OffPolicyTrainingConfig(total_steps=total, buffer_size=200 * T, batch_size=16 * T,
                                                warmstart_steps=20, evaluation_frequency=10),
        checkpoint=False, resume=False)


def test_compat_get_metrics(tmp_path):
    """MTSAC.get_metrics(Metrics.ALL, data): the full key set, equal to the engine-level values for the same eps;
    the enum's flag test picks the groups (NONE: {}; SRANK / DORMANT_NEURONS: their own keys)."""
    from mtrl.config.utils import Metrics
    from mtrl.rl.algorithms import MTSAC
    from mtrl.types import ReplayBufferSamples
    from mtrl_amd import netmetrics as NM

    T = 10
    exp = _experiment(tmp_path, T)
    agent = MTSAC.initialize(exp.algorithm, exp.env, seed=3)
    rng = np.random.default_rng(0)
    B = 16 * T
    o = np.zeros((B, 39 + T), np.float32)
    o[:, :39] = rng.standard_normal((B, 39))
    o[np.arange(B), 39 + np.arange(B) % T] = 1
    data = ReplayBufferSamples(o, rng.uniform(-1, 1, (B, 4)).astype(np.float32), o.copy(),
                               np.zeros((B, 1), np.float32), rng.uniform(0, 10, (B, 1)).astype(np.float32))
    rng_state = agent.rng_state()
    a2, logs = agent.get_metrics(Metrics.ALL, data)
    assert a2 is agent
    assert list(logs) == NM.expected_keys(3, 3, 2) and len(logs) == 33
    # the same eps at the engine level
    eps = np.random.default_rng()
    eps.bit_generator.state = rng_state
    e = eps.standard_normal((B, 4)).astype(np.float32)
    want = NM.compute_metrics(agent.engine, Metrics.ALL, o, e)
    assert logs == want
    for name in NM.member_names(2):
        total = sum(logs[f"metrics/dormant_neurons_{name}_torso_layer_{i}_count"] for i in range(3))
        assert logs[f"metrics/dormant_neurons_{name}_total_count"] == total
        assert logs[f"metrics/dormant_neurons_{name}_total_ratio"] == total / (3 * 64) * 100
        assert all(1 <= logs[f"metrics/srank_{name}_torso_layer_{i}"] <= 64 for i in range(3))
    assert agent.get_metrics(Metrics.NONE, data)[1] == {}
    assert set(agent.get_metrics(Metrics.SRANK, data)[1]) == {k for k in want if "srank" in k}
    assert set(agent.get_metrics(Metrics.DORMANT_NEURONS, data)[1]) == {k for k in want if "dormant" in k}
    agent.engine.close()


@pytest.mark.parametrize("switch", [None, "1"])
def test_trainer_calls_get_metrics_only_when_switched_on(tmp_path, monkeypatch, switch):
    from fake_env import FakeMTVecEnv
    from mtrl.config.utils import Metrics
    from mtrl.rl.algorithms import MTSAC

    if switch is None:
        monkeypatch.delenv("MTSAC_NETWORK_METRICS", raising=False)
    else:
        monkeypatch.setenv("MTSAC_NETWORK_METRICS", switch)
    calls = []
    real = MTSAC.get_metrics

    def spy(self, metrics, data):
        out = real(self, metrics, data)
        calls.append((metrics, len(out[1])))
        return out

    monkeypatch.setattr(MTSAC, "get_metrics", spy)
    T = 10
    agent = _experiment(tmp_path, T, total=T * 60).run(envs=FakeMTVecEnv(T, max_steps=7))
    agent.engine.close()
    if switch is None:
        assert calls == []
    else:
        assert calls and all(m is Metrics.ALL and k == 33 for m, k in calls)
