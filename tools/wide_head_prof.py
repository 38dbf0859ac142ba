"""Serialised eager steps of one engine with a wide action space (for rocprofv3 --kernel-trace --stats).
usage: wide_head_prof.py T n W A [precision: 0 fp32, 1 split3, 3 split2h] [steps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtrl_amd import _lib as L  # noqa: E402
from mtrl_amd.engine import MTSACEngine, make_config  # noqa: E402
from mtrl_amd.init import init_mtsac  # noqa: E402

T, n, W, A = (int(x) for x in sys.argv[1:5])
prec = int(sys.argv[5]) if len(sys.argv) > 5 else 3
steps = int(sys.argv[6]) if len(sys.argv) > 6 else 12
D = 39 + T
eng = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=D, action_dim=A, actor_width=W, critic_width=W,
                              batch_per_task=n, capacity=2000, precision=prec), device=0)
actor, critic = init_mtsac(T, D, A, W, 3, W, 3, 2, seed=1)
eng.set_params(L.ACTOR, actor)
eng.set_params(L.CRITIC, critic)
eng.set_params(L.CRITIC_TARGET, critic)
eng.buffer_fill_synthetic(1234)
eng.seed_rng(1)
eng.enable_graph(False)
eng.set_timing(True, serial=True)
eng.update_many(steps)
eng.synchronize()
print({k: round(v, 5) for k, v in eng.logs().items()})
eng.close()
