"""The guard-zone mode (MTSAC_GUARD_BYTES, engine.cpp alloc: 0xFF bytes around every device allocation)
over whole steps: a split-K workspace, plane buffer or partial-sum buffer sized too small for a launch
shows as a written guard (mtsac_debug_check_guards) instead of a device fault.  The cases are the
smallest shapes that reach each branch of the trunk GEMM builders (engine.cpp fwd_params, dgrad_params,
wgrad_params) and of the workspace sizing in mtsac_create that asks them: gemm_x3f with split-K (a task
shard), the weight-grad slabs in ws_wg (deferred finish) and in ws_lane (sharded), the narrow-trunk
kernels, one / two / three operand planes, padded extents that all differ from the logical ones, and a
trunk without hidden layers.  Which kernel each case runs on one MI355X: profiles/launch_params_refactor.txt.

The variable is read once per process, so every case runs in a child process started with it set: 2
device-sampled steps eagerly and 2 through the step graph, the guards and the logs checked after each pair."""

from __future__ import annotations

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GUARD_BYTES = 4096

# T (num_tasks), tc (task_count), width, depth, precision, rows per task, modelled collective
CASES = {
    "shard7_w2048_split2h": dict(T=50, tc=7, W=2048, depth=3, prec="split2h", n=128, model=False),
    "shard7_w2048_split2h_modelled": dict(T=50, tc=7, W=2048, depth=3, prec="split2h", n=128, model=True),
    "mt10_w400_split3": dict(T=10, tc=10, W=400, depth=3, prec="split3", n=128, model=False),
    "mt10_w2048_bf16": dict(T=10, tc=10, W=2048, depth=3, prec="bf16", n=128, model=False),
    "t3_w100_d2_split2h": dict(T=3, tc=3, W=100, depth=2, prec="split2h", n=5, model=False),
    "t2_w64_d1_split3": dict(T=2, tc=2, W=64, depth=1, prec="split3", n=8, model=False),
    "t2_w64_d1_fp32": dict(T=2, tc=2, W=64, depth=1, prec="fp32", n=8, model=False),
}


def make_engine(name):
    """The case's engine with init_mtsac parameters, a synthetic buffer and seeded streams."""
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config
    from mtrl_amd.init import init_mtsac

    c = CASES[name]
    T, tc, W, D = c["T"], c["tc"], c["W"], c["depth"]
    eng = MTSACEngine(make_config(num_tasks=T, task_begin=0, task_count=tc, obs_dim=39 + T, action_dim=4,
                                  actor_width=W, critic_width=W, actor_depth=D, critic_depth=D, num_critics=2,
                                  batch_per_task=c["n"], capacity=256, precision=L.PRECISIONS[c["prec"]]))
    actor, critic = init_mtsac(T, 39 + T, 4, W, D, W, D, 2, seed=3, task_begin=0, task_count=tc)
    eng.set_params(L.ACTOR, actor)
    eng.set_params(L.CRITIC, critic)
    eng.set_params(L.CRITIC_TARGET, critic)
    eng.buffer_fill_synthetic(99)
    eng.seed_rng(7)
    if c["model"]:
        L.check(eng.lib.mtsac_debug_set_collective_model(eng._h, 8, 300.0, 1))
    return eng


def check_guards(eng, tag):
    """Every guard zone intact (the report of the written ones printed otherwise), every log finite."""
    import math

    logs = eng.logs()  # synchronizes the steps
    bad = eng.lib.mtsac_debug_check_guards(eng._h)
    if bad != 0:
        print(f"{tag}: guards {bad}: {eng.lib.mtsac_last_error().decode()}", flush=True)
    assert bad == 0, (tag, bad)
    assert all(math.isfinite(v) for v in logs.values()), (tag, logs)


def run_steps(eng, name):
    eng.enable_graph(False)
    eng.update_many(2)
    check_guards(eng, name + "/eager")
    eng.enable_graph(True)
    eng.update_many(2)
    check_guards(eng, name + "/graph")


_CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_guards as t
eng = t.make_engine({name!r})
t.run_steps(eng, {name!r})
eng.close()
print("guards intact, logs finite")
"""


@pytest.mark.parametrize("name", list(CASES))
def test_steps_leave_every_guard_zone_intact(name):
    env = dict(os.environ, MTSAC_GUARD_BYTES=str(GUARD_BYTES))
    r = subprocess.run([sys.executable, "-u", "-c", _CHILD.format(root=ROOT, tests=TESTS, name=name)],
                       capture_output=True, text=True, timeout=200, env=env)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "guards intact" in r.stdout
