"""Time the network health metrics (MTSAC.get_metrics' pass) at a workload's full size on the device: the
whole network_metrics call (forward, kernels, copies of the results), the statistics and Gram kernels alone by
HIP events, and the host eigen solves that turn the Grams into srank.
usage: python tools/metrics_bench.py [T] [W] [reps] [precision]     (defaults: MT10/W400 then MT50/W2048)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mtrl_amd import _lib as L  # noqa: E402
from mtrl_amd import netmetrics as nm  # noqa: E402
from mtrl_amd.engine import MTSACEngine, make_config  # noqa: E402
from mtrl_amd.init import init_mtsac  # noqa: E402


def bench(T, W, reps, precision):
    e = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W,
                                batch_per_task=128, capacity=1000, precision=L.PRECISIONS[precision]))
    a, q = init_mtsac(T, 39 + T, 4, W, 3, W, 3, 2, seed=1)
    e.set_params(L.ACTOR, a)
    e.set_params(L.CRITIC, q)
    e.set_params(L.CRITIC_TARGET, q)
    e.buffer_fill_synthetic(7)
    e.seed_rng(1)
    e.network_metrics()  # warm-up (allocates the scratch)
    for _ in range(reps):
        t0 = time.perf_counter()
        out = e.network_metrics()
        t1 = time.perf_counter()
        stats_ms, gram_ms = e.network_metrics_kernel_ms()
        sr = {net: [[nm.srank_from_gram(g) for g in member] for member in out[net]["gram"]] for net in out}
        t2 = time.perf_counter()
        r = out["actor"]["gram"][0][0].shape[0]
        gflop = 9 * 2.0 * r * r * (128 * T if r == W else W) / 2 / 1e9  # one triangle, 3 layers x (1 + 2) members
        print(f"T={T} W={W} {precision}: whole call {1e3 * (t1 - t0):.1f} ms; statistics kernels {stats_ms:.3f} ms, "
              f"Gram kernels {gram_ms:.3f} ms ({gflop / max(gram_ms, 1e-9):.1f} TFLOP/s fp64 on r = {r}); host "
              f"eigvalsh of 9 Grams {1e3 * (t2 - t1):.1f} ms", flush=True)
    print("  dormant counts actor", out["actor"]["counts"].tolist(), "critic", out["critic"]["counts"].tolist(),
          "srank", sr, flush=True)
    e.close()


if __name__ == "__main__":
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    precision = sys.argv[4] if len(sys.argv) > 4 else "split2h"
    cases = [(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else [(10, 400), (50, 2048)]
    for T, W in cases:
        bench(T, W, reps, precision)
