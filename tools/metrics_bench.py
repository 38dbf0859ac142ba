"""Time the network health metrics (MTSAC.get_metrics' pass) at a workload's full size on the device: the
whole network_metrics call (forward, kernels, copies of the results), the statistics and Gram kernels alone by
HIP events, and the eigen solves that turn the Grams into srank: on the host (copies of the Grams, then
numpy.linalg.eigvalsh) or on the device (--eig device: the reduction and the bisection by HIP events, and the
launches of the solve).
usage: python tools/metrics_bench.py [T] [W] [reps] [precision] [--eig host|device]
       (defaults: MT10/W400 then MT50/W2048, --eig host)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from mtrl_amd import _lib as L  # noqa: E402
from mtrl_amd import netmetrics as nm  # noqa: E402
from mtrl_amd.engine import MTSACEngine, make_config  # noqa: E402
from mtrl_amd.init import init_mtsac  # noqa: E402


def gram_copies_ms(e, out):
    """The device-to-host copies of the nine Grams again, into the arrays the call filled."""
    t0 = time.perf_counter()
    for which, net in enumerate(("actor", "critic")):
        for m, member in enumerate(out[net]["gram"]):
            for i, g in enumerate(member):
                L.check(e.lib.mtsac_get_network_gram(e._h, which, m, i, g.ctypes.data))
    return 1e3 * (time.perf_counter() - t0)


def bench(T, W, reps, precision, eig="host"):
    e = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W,
                                batch_per_task=128, capacity=1000, precision=L.PRECISIONS[precision]))
    a, q = init_mtsac(T, 39 + T, 4, W, 3, W, 3, 2, seed=1)
    e.set_params(L.ACTOR, a)
    e.set_params(L.CRITIC, q)
    e.set_params(L.CRITIC_TARGET, q)
    e.buffer_fill_synthetic(7)
    e.seed_rng(1)
    e.network_metrics(eig=eig)  # warm-up (allocates the scratch)
    for _ in range(reps):
        t0 = time.perf_counter()
        out = e.network_metrics(eig=eig)
        t1 = time.perf_counter()
        stats_ms, gram_ms = e.network_metrics_kernel_ms()
        if eig == "host":
            sr = {net: [[nm.srank_from_gram(g) for g in member] for member in out[net]["gram"]] for net in out}
            t2 = time.perf_counter()
            r = out["actor"]["gram"][0][0].shape[0]
            tail = (f"Gram copies {gram_copies_ms(e, out):.1f} ms (inside the whole call); host eigvalsh of 9 Grams "
                    f"{1e3 * (t2 - t1):.1f} ms")
        else:
            sr = {net: [[nm.srank_from_singular_values(nm.singular_values_from_eigvals(lam)) for lam in member]
                        for member in out[net]["eigvals"]] for net in out}
            t2 = time.perf_counter()
            r = out["actor"]["eigvals"].shape[-1]
            ms = [e.network_eigvals_kernel_ms(which) for which in (0, 1)]
            tail = (f"no Gram copies; device reduction {ms[0][0] + ms[1][0]:.1f} ms, bisection "
                    f"{ms[0][1] + ms[1][1]:.1f} ms, {ms[0][2] + ms[1][2]} launches (inside the whole call); host "
                    f"srank from the eigenvalues {1e3 * (t2 - t1):.1f} ms")
        gflop = 9 * 2.0 * r * r * (128 * T if r == W else W) / 2 / 1e9  # one triangle, 3 layers x (1 + 2) members
        print(f"T={T} W={W} {precision} eig={eig}: to srank {1e3 * (t2 - t0):.1f} ms; whole call "
              f"{1e3 * (t1 - t0):.1f} ms; statistics kernels {stats_ms:.3f} ms, "
              f"Gram kernels {gram_ms:.3f} ms ({gflop / max(gram_ms, 1e-9):.1f} TFLOP/s fp64 on r = {r}); {tail}",
              flush=True)
    print("  dormant counts actor", out["actor"]["counts"].tolist(), "critic", out["critic"]["counts"].tolist(),
          "srank", sr, flush=True)
    e.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    eig = "host"
    if "--eig" in argv:
        k = argv.index("--eig")
        eig = argv[k + 1]
        del argv[k:k + 2]
    if eig not in ("host", "device"):
        sys.exit("--eig host|device")
    reps = int(argv[2]) if len(argv) > 2 else 3
    precision = argv[3] if len(argv) > 3 else "split2h"
    cases = [(int(argv[0]), int(argv[1]))] if len(argv) > 1 else [(10, 400), (50, 2048)]
    for T, W in cases:
        bench(T, W, reps, precision, eig)
