#!/usr/bin/env python3
"""Time the shared-head (Vanilla, MTSAC_NET_SHARED_HEAD) step beside the multi-head step of the same tree.

Configurations: MT10/W400 B = 1280 and MT50/W2048 B = 6400, precision split2h, device-sampled batches and
device noise.  Default mode: per configuration two engines (shared head, multi-head), and per repeat,
alternating, a host clock around update_many(K) + synchronize after a warm-up; one line per engine with
the ms per step of every repeat.

Kernel times: ``--profile-steps N`` runs N shared-head steps per configuration and nothing else, for

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python tools/shared_head_bench.py --profile-steps 30

whose ``*_kernel_stats.csv`` lists head_bwd_weight_shared_kernel / head_shared_finish_kernel (one launch of
each per network per step) beside the step's other kernels.
Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

CONFIGS = {"mt10_w400": (10, 400), "mt50_w2048": (50, 2048)}


def engine(T: int, W: int, shared: bool):
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config
    from mtrl_amd.init import init_mtsac, init_vanilla

    c = make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W, batch_per_task=128,
                    capacity=2048, precision=L.FP32_SPLIT2H)
    e = MTSACEngine(c, shared_head=shared)
    a, q = (init_vanilla if shared else init_mtsac)(T, 39 + T, 4, W, 3, W, 3, 2, seed=1)
    e.set_params(L.ACTOR, a)
    e.set_params(L.CRITIC, q)
    e.set_params(L.CRITIC_TARGET, q)
    e.buffer_fill_synthetic(1234)
    e.seed_rng(1)
    return e


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--profile-steps", type=int, default=0)
    args = ap.parse_args()
    for name in args.configs.split(","):
        T, W = CONFIGS[name]
        if args.profile_steps:
            e = engine(T, W, True)
            e.update_many(args.profile_steps)
            e.synchronize()
            e.close()
            continue
        engs = {"shared": engine(T, W, True), "multi": engine(T, W, False)}
        for e in engs.values():
            e.update_many(args.warmup)
            e.synchronize()
        res = {k: [] for k in engs}
        for _ in range(args.repeats):
            for k, e in engs.items():
                e.synchronize()
                t0 = time.perf_counter()
                e.update_many(args.steps)
                e.synchronize()
                res[k].append((time.perf_counter() - t0) / args.steps * 1e3)
        for k, v in res.items():
            print(f"{name} split2h {k:6s} ms/step: " + "  ".join(f"{x:.4f}" for x in v), flush=True)
        for e in engs.values():
            e.close()


if __name__ == "__main__":
    main()
