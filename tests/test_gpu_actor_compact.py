"""The actor step's pass through the critic over each member's active rows only (engine.cpp actor_compact:
active_rows -> compacted head backward -> gemm_x3f_ragged data grads -> action grad from the slots) against
the dense pass it replaces (mtsac_debug_set_actor_dense(1)).  The rows it drops are exactly zero in the
dense pass, and rows are independent, so nothing may differ: after 3 update_many steps the parameters
(actor, critic, target, log_alpha), the Adam moments and the logs are compared bit for bit, eager and graph.

T = 20, width 2048, 128 rows per task, split2h: 13 row tiles x 8 x 2 = 208 workgroups per data grad, so the
dense pass is the plain unsplit gemm_x3f launch and the compacted pass is taken.  `all_ties` sets critic
member 1 equal to member 0: every row is in both lists (cnt = 2), the worst-case grid, and the members stay
equal through the updates."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, W, N_PER_TASK, DEPTH, E, A = 20, 2048, 128, 3, 2, 4
STATE = list(range(10))  # _lib.ACTOR .. ALPHA_ADAM_NU
_init = {}


def _critic_leaves():
    from mtrl_amd.init import leaf_shapes

    return leaf_shapes(A + 39 + T, W, DEPTH, T, 1, E)


def _members(flat):
    """the flat critic (flax leaf order, every leaf [E][...]) as a list of [E][n] views"""
    out, off = [], 0
    for _, shape in _critic_leaves():
        n = int(np.prod(shape))
        out.append(flat[off:off + n].reshape(E, n // E))
        off += n
    assert off == flat.size
    return out


def _params(ties):
    if not _init:
        from mtrl_amd.init import init_mtsac

        _init["actor"], _init["critic"] = init_mtsac(T, 39 + T, A, W, DEPTH, W, DEPTH, E, seed=1)
    critic = _init["critic"].copy()
    if ties:
        for leaf in _members(critic):
            leaf[1] = leaf[0]
    return _init["actor"], critic


def _run(dense, graph, ties):
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config

    lib = L.load()
    L.check(lib.mtsac_debug_set_actor_dense(1 if dense else 0))  # read at engine creation
    try:
        cfg = make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W,
                          batch_per_task=N_PER_TASK, capacity=512, precision=L.FP32_SPLIT2H)
        eng = MTSACEngine(cfg)
    finally:
        L.check(lib.mtsac_debug_set_actor_dense(-1))
    actor, critic = _params(ties)
    eng.set_params(L.ACTOR, actor)
    eng.set_params(L.CRITIC, critic)
    eng.set_params(L.CRITIC_TARGET, critic)
    eng.buffer_fill_synthetic(1234)
    eng.seed_rng(1)
    eng.enable_graph(graph)
    eng.update_many(3)
    out = {w: eng.get_params(w) for w in STATE}
    out["logs"] = eng.logs()
    assert lib.mtsac_debug_actor_compact(eng._h) == (0 if dense else 1)  # the path under test was taken
    eng.close()
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("ties", [False, True], ids=["min", "all_ties"])
def test_compacted_actor_pass_is_bitwise_the_dense_one(graph, ties):
    from mtrl_amd import _lib as L

    new = _run(False, graph, ties)
    old = _run(True, graph, ties)
    print("logs compacted", new["logs"], "dense", old["logs"])
    assert new["logs"] == old["logs"]
    for w in STATE:
        np.testing.assert_array_equal(new[w].view(np.uint32), old[w].view(np.uint32), err_msg=f"state {w}")
    assert np.all(np.isfinite(new[L.ACTOR])) and np.any(new[L.ACTOR] != _init["actor"])  # the steps did something
    if ties:
        for which in (L.CRITIC, L.CRITIC_TARGET):
            for leaf in _members(new[which]):
                np.testing.assert_array_equal(leaf[0].view(np.uint32), leaf[1].view(np.uint32))
