"""The device noise stream (mtrl_amd/csrc/devrng.h normal4: Philox4x32-10 + Box-Muller) as the policy heads draw
it, against the host model of tests/philox_ref.py.

mtsac_debug_head_policy_noise runs the policy-head launches with eps == NULL; the drawn noise comes back in
cache[:, 4A:5A] and must equal normal4(seed, stream + 16 (j >> 2), counter, b // noise_div or b)[j & 3] within
philox_ref.normal_bound = (3 + 4 + 2) 2^-23 max(r, 1), r = sqrt(-2 ln u1): the model is evaluated in float64 at the
device's own float32 arguments, so what is left is the device's logf (3 ulp), cosf / sinf (4 ulp) and two
roundings.  A wrong word, lane, stream, row or counter moves a value by O(1).  The rest of the launch must be,
bit for bit, what the same entry gives with that noise injected.

Measured on an MI355X over every case below: the largest |device - model| / bound is printed by each test (0.156,
at the A = 19 head; recorded in DESIGN.md).  A ratio above 1 would be a finding, not a reason to move the bound.

The engine tests read the actor-loss pass's cache after device-noise steps (mtsac_debug_read id 5): stream 2 of
the plain step, stream 6 with one draw per row index shared by the tasks under PCGrad, at the counter
noise_state() reported before the step."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import philox_ref as P
import sac_head_cases as C
import test_gpu_head_kernels as K

pytestmark = pytest.mark.gpu

f32 = np.float32
W = 8
COUNTS = [(1,), (3, 4), (20, 0, 44)]  # B = 1, 7, 64
STREAMS = tuple(range(1, 9))
COUNTERS = (0, 1, 2**32 + 5)
SEED = 0x9E3779B97F4A7C15  # both key words in use
A_NARROW, A_WIDE = (1, 3, 4), (5, 19, 64)


@functools.lru_cache(maxsize=None)
def _model(seed, stream, counter, B, A, noise_div):
    return P.policy_eps(seed, stream, counter, B, A, noise_div)


def run_policy_noise(c, form, seed, stream, counter, noise_div, pad=3):
    A, B, T_l = c["A"], c["B"], c["T_l"]
    ns, ld = (2 if form == 2 else 1), A + pad
    h = K._in(c["h"][:ns])
    o = dict(a=K._nan(ns, B, ld), a2=K._nan(ns, B, ld), logpi=K._nan(ns, B), cache=K._nan(ns, B, 5 * A))
    counts, rows = np.zeros(T_l, np.int32), np.zeros((T_l, B), np.int32)
    K._check(K._lib().mtsac_debug_head_policy_noise(
        form, 0, B, T_l, c["W"], A, ld, K._p(c["task"]), K._p(h), K._p(c["Wh"]), K._p(c["bh"]), seed, stream, counter,
        noise_div, C.LS_MIN, C.LS_MAX, K._p(o["a"]), K._p(o["a2"]), K._p(o["logpi"]), K._p(o["cache"]), None,
        K._p(counts), K._p(rows)))
    K._lists_ok(c["task"], T_l, counts, rows)
    return o


def _check_case(c, form, stream, counter, noise_div):
    """-> the largest |device - model| / bound of the launch's noise."""
    A, B = c["A"], c["B"]
    got = run_policy_noise(c, form, SEED, stream, counter, noise_div)
    ns = 2 if form == 2 else 1
    eps = got["cache"][:, :, 4 * A:]
    worst = 0.0
    for s in range(ns):
        want, rad = _model(SEED, stream + s, counter, B, A, noise_div)
        err, bound = np.abs(eps[s].astype(np.float64) - want), P.normal_bound(rad)
        where = (form, A, B, stream, counter, noise_div, s)
        print(f"noise form={form} A={A} B={B} stream={stream + s} counter={counter} div={noise_div}: "
              f"max err / bound {float((err / bound).max()):.3f}")
        assert np.isfinite(eps[s]).all() and (err <= bound).all(), (where, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    # the same launch with the drawn noise injected: every output bit for bit
    inj = dict(c)
    e2 = np.zeros((2, B, A), f32)
    e2[:ns] = eps
    inj["eps"] = e2
    ref = K.run_policy(inj, form)
    for k in ("a", "a2", "logpi", "cache"):
        assert K._same(got[k], ref[k]), (k, "differs from the launch with the same noise injected", form, A, B)
    return worst


@pytest.mark.parametrize("A", A_NARROW + A_WIDE)
def test_policy_heads_draw_the_model_stream(A):
    worst, i = 0.0, A
    for counts in COUNTS:
        c = C.policy_case(A, W, counts)
        for form in (0, 1, 2):
            for noise_div in (0, c["T_l"]):
                i += 1
                worst = max(worst, _check_case(c, form, STREAMS[i % 8], COUNTERS[i % 3], noise_div))
    print(f"device noise A={A}: worst err / bound {worst:.3f}")


def test_every_stream_and_counter():
    """Stream ids 1 .. 8 x the counters (0, 1, past 2^32) x row sharing at one narrow and one wide head."""
    worst = 0.0
    for A in (4, 5):
        c = C.policy_case(A, W, COUNTS[1])
        for stream in STREAMS:
            for counter in COUNTERS:
                for noise_div in (0, c["T_l"]):
                    worst = max(worst, _check_case(c, 1, stream, counter, noise_div))
    print(f"device noise, streams x counters: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------ the engine's own steps
def _engine(pcgrad):
    from mtrl_amd.engine import MTSACEngine, make_config
    from oracle import mtsac as om

    import test_gpu_update as U

    T, Wd, n = 3, 16, 4
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, actor_width=Wd, critic_width=Wd)
    eng = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=Wd, critic_width=Wd,
                                  batch_per_task=n, capacity=64, precision=1 if pcgrad else 0))
    if pcgrad:
        eng.set_pcgrad(True)
    U._load_state(eng, U._f32_state(cfg, seed=2))
    eng.buffer_fill_synthetic(7)
    eng.seed_rng(1)
    return eng, T, n


@pytest.mark.parametrize("pcgrad", [False, True], ids=["plain", "pcgrad"])
def test_engine_steps_draw_the_model_stream(pcgrad):
    """Three device-noise steps: the cached eps of the actor-loss pass is the model's at the step's counter."""
    eng, T, n = _engine(pcgrad)
    B, A = n * T, 4
    seed, c0 = eng.noise_state()
    stream, div = (6, T) if pcgrad else (2, 0)
    worst = 0.0
    for k in range(3):
        eng.update_many(1)
        cache = np.empty((B, 5 * A), f32)
        K._check(eng.lib.mtsac_debug_read(eng._h, 5, K._p(cache), cache.size))
        want, rad = P.policy_eps(seed, stream, c0 + k, B, A, div)
        err, bound = np.abs(cache[:, 4 * A:].astype(np.float64) - want), P.normal_bound(rad)
        print(f"engine noise pcgrad={pcgrad} step {k}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (k, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        if pcgrad:  # rows i T + t share the draw of i
            e = cache[:, 4 * A:].reshape(n, T, A)
            assert all(K._same(e[:, t], e[:, 0]) for t in range(T))
    assert eng.noise_state() == (seed, c0 + 3)
    eng.close()
