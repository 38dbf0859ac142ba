"""The device eigen solve inside the engine (mtsac_network_eigvals, eig="device"): the whole metrics path against
the float64 oracle, the getter contract around the consumed Grams, no side effects on training, and the compat
layer's MTSAC_NETWORK_METRICS_EIG switch.  Statements and bars: tests/network_metrics_ref.py, tests/symeig_ref.py."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import network_metrics_ref as R
import symeig_ref as S

pytestmark = pytest.mark.gpu

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
def test_whole_path_device_eigvals(shape, precision):
    """srank exact against the float64 forward's SVD (the reference's margins asserted first); the eigenvalues
    within the C_EIG bar of eigvalsh of the same Grams, fetched from an identical eig="host" call; the dormant
    results byte-identical to that call's."""
    from mtrl_amd import netmetrics as NM

    (cfg, actor, critic, obs, eps), exp, ok = _expect(shape)
    assert ok, "the float64 reference must keep its margins from 0.1 and from 0.99 (tests/network_metrics_ref.py)"
    T, n, W, D, A, E = shape
    r = min(n * T, W)
    eng = _engine(shape, precision, actor, critic)
    try:
        dev = eng.network_metrics(obs, eps, eig="device")
        host = eng.network_metrics(obs, eps, eig="host")
    finally:
        eng.close()
    worst = 0.0
    for name, rows in exp.items():
        net = "actor" if name == "actor" else "critic"
        e = 0 if name == "actor" else int(name.split("_")[1])
        assert dev[net]["gram"] is None and dev[net]["eigvals"].shape == (dev[net]["members"], D, r)
        assert not dev[net]["eig_flags"].any()
        assert dev[net]["scores"].tobytes() == host[net]["scores"].tobytes()
        assert dev[net]["counts"].tobytes() == host[net]["counts"].tobytes()
        for i, want in enumerate(rows):
            lam = dev[net]["eigvals"][e][i]
            assert NM.srank_from_singular_values(NM.singular_values_from_eigvals(lam)) == want["srank"], (name, i)
            ref = np.linalg.eigvalsh(host[net]["gram"][e][i])
            assert np.all(np.diff(lam) >= 0)
            worst = max(worst, S.ratio(lam, ref))
            assert np.max(np.abs(lam - ref)) <= S.bar(r, ref), (name, i, worst)
    print(f"device eigvals {shape} {precision}: worst err / (r 2^-52 max|ref|) = {worst:.3g} of C_EIG = {S.C_EIG}")


def test_getter_contract():
    """network_eigvals needs the Grams of a call with bit 1 and consumes them; the next metrics call restores
    both getters."""
    from mtrl_amd._lib import MTSACError

    shape = (3, 5, 36, 3, 4, 2)
    (cfg, actor, critic, obs, eps), _, _ = _expect(shape)
    eng = _engine(shape, "split2h", actor, critic)
    G = np.empty((15, 15))

    def gram(which):
        return eng.lib.mtsac_get_network_gram(eng._h, which, 0, 0, G.ctypes.data)

    try:
        with pytest.raises(MTSACError, match="-22"):
            eng.network_eigvals(0)
        eng.network_metrics(obs, eps, dormant=True, gram=False)
        with pytest.raises(MTSACError, match="-22"):
            eng.network_eigvals(1)
        eng.network_metrics(obs, eps)
        assert gram(0) == 0 and gram(1) == 0
        lam, flags = eng.network_eigvals(1)
        assert lam.shape == (2, 3, 15) and flags.shape == (2, 3) and not flags.any()
        assert gram(1) == -22 and b"consumed" in eng.lib.mtsac_last_error()
        assert gram(0) == 0  # the actor's Grams are still there
        with pytest.raises(MTSACError, match="-22"):
            eng.network_eigvals(1)
        lam_a, _ = eng.network_eigvals(0)
        assert gram(0) == -22
        again = eng.network_metrics(obs, eps)
        assert gram(0) == 0 and gram(1) == 0
        lam2, _ = eng.network_eigvals(1)
        assert lam2.tobytes() == lam.tobytes()
        ref = np.linalg.eigvalsh(again["actor"]["gram"][0][0])
        assert np.max(np.abs(lam_a[0][0] - ref)) <= S.bar(15, ref)
        assert eng.lib.mtsac_network_eigvals(eng._h, 2, lam.ctypes.data, flags.ctypes.data) == -22
        assert eng.lib.mtsac_network_eigvals(eng._h, 0, None, flags.ctypes.data) == -22
    finally:
        eng.close()


def test_sharded_engine_refuses():
    from mtrl_amd._lib import MTSACError
    from mtrl_amd.engine import MTSACEngine, make_config

    e = MTSACEngine(make_config(num_tasks=4, task_begin=2, task_count=2, obs_dim=43, actor_width=32, critic_width=32,
                                batch_per_task=4, capacity=64, precision=1))
    try:
        with pytest.raises(MTSACError, match="-95"):
            e.network_eigvals(0)
    finally:
        e.close()


def _state(eng):
    return [eng.get_params(w).tobytes() for w in range(10)] + [eng.get_adam_count(i) for i in range(3)] + \
        [np.array(list(eng.logs().values()), np.float32).tobytes(), eng.noise_state()]


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_no_side_effects_between_updates(mode):
    """Two engines from one state; one runs compute_metrics(..., eig="device") between two updates: parameters,
    Adam moments, counts, logs and the noise stream stay bitwise equal."""
    from helpers import synthetic_batch, synthetic_eps
    from mtrl_amd import netmetrics as NM
    from mtrl_amd.compat.config.utils import Metrics

    shape = (3, 5, 36, 3, 4, 2)
    T, n, W, D, A, E = shape
    (cfg, actor, critic, obs, eps), _, _ = _expect(shape)
    engines = [_engine(shape, "split2h", actor, critic, noise_seed=9) for _ in range(2)]
    try:
        states = []
        for k, eng in enumerate(engines):
            if mode == "graph":
                eng.buffer_fill_synthetic(3)
                eng.seed_rng(5)
                eng.enable_graph(True)
                eng.update_many(2)
            else:
                b1 = synthetic_batch(T, n * T, action_dim=A, seed=1, dtype=np.float32)
                eng.update(b1, *synthetic_eps(n * T, action_dim=A, seed=2, dtype=np.float32))
            if k == 1:
                logs = NM.compute_metrics(eng, Metrics.ALL, obs, eps, eig="device")
                assert list(logs) == NM.expected_keys(D, D, E)
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


def test_compute_metrics_device_equals_host():
    """The LogDict of a whole-path case: eig="device" and eig="host" give the same keys and the same values."""
    from mtrl_amd import netmetrics as NM
    from mtrl_amd.compat.config.utils import Metrics

    shape = (10, 13, 132, 2, 6, 1)
    (cfg, actor, critic, obs, eps), _, ok = _expect(shape)
    assert ok
    eng = _engine(shape, "split2h", actor, critic)
    try:
        host = NM.compute_metrics(eng, Metrics.ALL, obs, eps)
        dev = NM.compute_metrics(eng, Metrics.ALL, obs, eps, eig="device")
        only = NM.compute_metrics(eng, Metrics.SRANK, obs, eps, eig="device")
        none = NM.compute_metrics(eng, Metrics.DORMANT_NEURONS, obs, eps, eig="device")
    finally:
        eng.close()
    assert list(dev) == list(host) and dev == host
    assert only == {k: v for k, v in host.items() if "srank" in k}
    assert none == {k: v for k, v in host.items() if "dormant" in k}


def test_trainer_switch(tmp_path, monkeypatch):
    """MTSAC.get_metrics with MTSAC_NETWORK_METRICS_EIG=device: the same LogDict as the default for the same
    noise (same keys, same integers), and a bad value is refused."""
    from fake_env import FakeMetaworldConfig
    from mtrl.config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
    from mtrl.config.nn import MultiHeadConfig
    from mtrl.config.optim import OptimizerConfig
    from mtrl.config.utils import Metrics
    from mtrl.rl.algorithms import MTSAC, MTSACConfig
    from mtrl.types import ReplayBufferSamples
    from mtrl_amd import netmetrics as NM

    T, W, n = 10, 36, 5
    algo = MTSACConfig(
        num_tasks=T, gamma=0.99,
        actor_config=ContinuousActionPolicyConfig(network_config=MultiHeadConfig(
            num_tasks=T, width=W, optimizer=OptimizerConfig(max_grad_norm=1.0))),
        critic_config=QValueFunctionConfig(network_config=MultiHeadConfig(
            num_tasks=T, width=W, optimizer=OptimizerConfig(max_grad_norm=1.0))),
        num_critics=2)
    agent = MTSAC.initialize(algo, FakeMetaworldConfig(env_id="MT10"), seed=3)
    rng = np.random.default_rng(0)
    B = n * T
    o = np.zeros((B, 39 + T), np.float32)
    o[:, :39] = rng.standard_normal((B, 39))
    o[np.arange(B), 39 + np.arange(B) % T] = 1
    data = ReplayBufferSamples(o, rng.uniform(-1, 1, (B, 4)).astype(np.float32), o.copy(),
                               np.zeros((B, 1), np.float32), rng.uniform(0, 10, (B, 1)).astype(np.float32))
    try:
        st = agent.rng_state()
        monkeypatch.delenv("MTSAC_NETWORK_METRICS_EIG", raising=False)
        _, host = agent.get_metrics(Metrics.ALL, data)
        agent.set_rng_state(st)
        monkeypatch.setenv("MTSAC_NETWORK_METRICS_EIG", "device")
        calls = []
        real = agent.engine.network_eigvals
        monkeypatch.setattr(agent.engine, "network_eigvals", lambda which: calls.append(which) or real(which))
        _, dev = agent.get_metrics(Metrics.ALL, data)
        assert calls == [0, 1]  # the device solve ran
        assert list(dev) == NM.expected_keys(3, 3, 2) and list(dev) == list(host)
        assert dev == host
        assert all(isinstance(v, int) for k, v in dev.items() if "srank" in k or k.endswith("_count"))
        monkeypatch.setenv("MTSAC_NETWORK_METRICS_EIG", "cpu")
        with pytest.raises(ValueError):
            agent.get_metrics(Metrics.ALL, data)
    finally:
        agent.engine.close()
