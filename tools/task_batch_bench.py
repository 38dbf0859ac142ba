#!/usr/bin/env python3
"""Time the plain step on per-task batch sizes (mtsac_set_task_batch_sizes) beside the balanced step of the same tree.

Configurations: MT10/W400 B = 1280 and MT50/W2048 B = 6400, precision split2h, device-sampled batches and device
noise.  Per configuration four engines -- balanced; mildly uneven sizes (alternating 1.25 n and 0.75 n); extreme
ones (task 0 holds half the batch, the others share the rest); the mild sizes with the per-task loss reduction on
(mtsac_set_task_loss_logging) -- and per repeat, alternating, a host clock around update_many(K) + synchronize
after a warm-up; one line per engine with the ms per step of every repeat.

Kernel times: ``--profile-steps N`` runs N steps of ``--profile-kind`` (default: the extreme sizes) with the loss
reduction on per configuration and nothing else, for

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python tools/task_batch_bench.py --profile-steps 30

whose ``*_kernel_stats.csv`` lists replay_indices_tasks_kernel, the task-major gather_kernel<2> and
task_losses_rows_kernel (one launch of each per step) beside the step's other kernels.
Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

CONFIGS = {"mt10_w400": (10, 400), "mt50_w2048": (50, 2048)}
N = 128


def sizes_of(kind: str, T: int):
    B = N * T
    if kind == "mild":
        s = np.array([N + N // 4, N - N // 4] * (T // 2) + [N] * (T % 2))
    else:  # extreme
        rest, k = B - B // 2, T - 1
        s = np.array([B // 2] + [rest // k + (1 if i < rest % k else 0) for i in range(k)])
    assert s.sum() == B and len(s) == T
    return s.astype(np.int32)


def engine(T: int, W: int, kind: str, logging: bool, graph: bool):
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config
    from mtrl_amd.init import init_mtsac

    c = make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W, batch_per_task=N,
                    capacity=4096, precision=L.FP32_SPLIT2H)
    e = MTSACEngine(c)
    a, q = init_mtsac(T, 39 + T, 4, W, 3, W, 3, 2, seed=1)
    e.set_params(L.ACTOR, a)
    e.set_params(L.CRITIC, q)
    e.set_params(L.CRITIC_TARGET, q)
    e.buffer_fill_synthetic(1234)
    e.seed_rng(1)
    e.enable_graph(graph)
    if kind != "balanced":
        e.set_task_batch_sizes(sizes_of(kind, T))
    if logging:
        e.set_task_loss_logging(True)
    return e


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--eager", action="store_true", help="eager issue instead of hipGraph replay")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--profile-kind", default="extreme", choices=["balanced", "mild", "extreme"])
    args = ap.parse_args()
    for name in args.configs.split(","):
        T, W = CONFIGS[name]
        if args.profile_steps:
            e = engine(T, W, args.profile_kind, True, False)
            e.update_many(args.profile_steps)
            e.synchronize()
            e.close()
            continue
        engs = {"balanced": engine(T, W, "balanced", False, not args.eager),
                "mild": engine(T, W, "mild", False, not args.eager),
                "extreme": engine(T, W, "extreme", False, not args.eager),
                "mild+losses": engine(T, W, "mild", True, not args.eager)}
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
            print(f"{name} split2h {'eager' if args.eager else 'graph'} {k:12s} ms/step: " +
                  "  ".join(f"{x:.4f}" for x in v), flush=True)
        for e in engs.values():
            e.close()


if __name__ == "__main__":
    main()
