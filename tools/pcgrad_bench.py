#!/usr/bin/env python3
"""Time the PCGrad training step beside the plain eager step, and its Gram / combine kernels.

Configurations: MT10/W400 B = 1280 (experiments/misc/mt10_mtmhsac_pcgrad.py) and MT50/W2048 B = 6400.

Step times (default mode): per configuration and repeat, alternating, K plain eager steps and K PCGrad
steps (device-sampled batches, device noise, device-drawn task orders), each a host clock around
update_many(K) + synchronize, after a warm-up.  One JSON line per configuration.

Kernel times: run the PCGrad steps alone under the profiler, in a run of its own,

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python tools/pcgrad_bench.py --profile-steps 20 --configs mt50_w2048

then ``--stats-csv OUT/.../*_kernel_stats.csv --configs mt50_w2048`` turns the per-kernel averages of
gram_kernel / combine_kernel (one launch per network per step) into achieved bytes/s over
(T P + P) 4 bytes per launch, against the 6.29 TB/s float4-copy rate (MI355X_MICROARCH.md).
``--surgery cagrad`` adds the CAGrad step on a third engine of the same tree: the
three steps alternate within every repeat, ``--profile-steps`` runs CAGrad steps, and the kernel table
lists cagrad_solve_kernel beside pcgrad_solve_kernel.
``--surgery gradnorm`` does the same with the GradNorm step as a fourth engine: plain,
PCGrad, CAGrad and GradNorm alternate within every repeat, and the kernel table lists gradnorm_solve_kernel
and task_losses_kernel too.
Needs the GPU (except --stats-csv): there is no fallback.
"""

from __future__ import annotations

import argparse
import csv
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

COPY_RATE = 6.29e12  # bytes/s, float4 copy (MI355X_MICROARCH.md)
CONFIGS = {"mt10_w400": (10, 400, 128), "mt50_w2048": (50, 2048, 128)}


def param_counts(T, W, depth=3, A=4, E=2):
    """(critic P, actor P) of the multi-head MLPs (flax ravel size)."""
    def net(in_dim, hd, e):
        return e * (T * hd + T * W * hd + depth * W + in_dim * W + (depth - 1) * W * W)
    return net(39 + T + A, 1, E), net(39 + T, 2 * A, 1)


def make_engine(T, W, n, precision, surgery):
    """surgery: None (the plain eager step), "pcgrad", "cagrad" or "gradnorm"."""
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config
    from mtrl_amd.init import init_mtsac

    e = MTSACEngine(make_config(num_tasks=T, task_count=T, obs_dim=39 + T, actor_width=W, critic_width=W,
                                batch_per_task=n, capacity=2000, precision=L.PRECISIONS[precision]))
    a, q = init_mtsac(T, 39 + T, 4, W, 3, W, 3, 2, seed=1)
    e.set_params(L.ACTOR, a)
    e.set_params(L.CRITIC, q)
    e.set_params(L.CRITIC_TARGET, q)
    e.buffer_fill_synthetic(7)
    e.seed_rng(1)
    e.enable_graph(False)
    if surgery:
        {"pcgrad": e.set_pcgrad, "cagrad": e.set_cagrad, "gradnorm": e.set_gradnorm}[surgery](True)
        assert (e.task_gradient_size(0), e.task_gradient_size(1)) == param_counts(T, W)
    return e


def time_steps(e, steps):
    e.synchronize()
    t0 = time.perf_counter()
    e.update_many(steps)
    e.synchronize()
    return (time.perf_counter() - t0) / steps


def spread(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs)}


def kernel_rates(stats_csv, T, W):
    """Achieved bytes/s of the Gram and combine kernels from a rocprofv3 kernel-stats CSV of PCGrad steps
    at this configuration: one launch per network per step, so the mean launch moves the mean of the two
    networks' (T P + P) 4 bytes."""
    pc_, pa_ = param_counts(T, W)
    mean_bytes = ((T + 1) * pc_ + (T + 1) * pa_) * 4 / 2
    out = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            for key in ("gram_kernel", "combine_kernel", "gram_sum_kernel", "pcgrad_solve_kernel",
                        "cagrad_solve_kernel", "gradnorm_solve_kernel", "task_losses_kernel"):
                if f"::{key}" in row["Name"] or row["Name"].startswith(key):
                    avg = float(row["AverageNs"]) * 1e-9
                    out[key] = {"calls": int(row["Calls"]), "avg_us": 1e6 * avg}
                    if key in ("gram_kernel", "combine_kernel"):
                        out[key] |= {"bytes_per_s": mean_bytes / avg, "of_copy_rate": mean_bytes / avg / COPY_RATE}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--precision", default="split2h")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--surgery", default="pcgrad", choices=["pcgrad", "cagrad", "gradnorm"],
                    help="cagrad: time the CAGrad step too, alternating with the other two; gradnorm: the CAGrad "
                         "and the GradNorm step too")
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="only run this many steps of --surgery's kind (for rocprofv3)")
    ap.add_argument("--stats-csv", default=None, help="rocprofv3 kernel-stats CSV of a --profile-steps run")
    args = ap.parse_args()

    for name in args.configs:
        T, W, n = CONFIGS[name]
        if args.stats_csv:
            print(json.dumps({"config": name, "kernels": kernel_rates(args.stats_csv, T, W)}), flush=True)
            continue
        if args.profile_steps:
            e = make_engine(T, W, n, args.precision, args.surgery)
            e.update_many(args.profile_steps)
            e.synchronize()
            e.close()
            continue
        pc = make_engine(T, W, n, args.precision, "pcgrad")
        plain = make_engine(T, W, n, args.precision, None)
        ca = make_engine(T, W, n, args.precision, "cagrad") if args.surgery in ("cagrad", "gradnorm") else None
        gn = make_engine(T, W, n, args.precision, "gradnorm") if args.surgery == "gradnorm" else None
        plain.update_many(args.warmup)
        pc.update_many(args.warmup)
        if ca:
            ca.update_many(args.warmup)
        if gn:
            gn.update_many(args.warmup)
        tp, tq, tc, tg = [], [], [], []
        for _ in range(args.repeats):
            tp.append(time_steps(plain, args.steps))
            tq.append(time_steps(pc, args.steps))
            if ca:
                tc.append(time_steps(ca, args.steps))
            if gn:
                tg.append(time_steps(gn, args.steps))
        logs = pc.logs() | pc.pcgrad_logs()
        if ca:
            logs |= {k: v for k, v in ca.cagrad_logs().items() if np.ndim(v) == 0}
        out = {
            "config": name, "T": T, "width": W, "batch": n * T, "precision": args.precision, "steps": args.steps,
            "plain_eager_step": spread(tp), "pcgrad_step": spread(tq),
            "ratio_pcgrad_over_plain": statistics.median(tq) / statistics.median(tp),
            "critic_P": pc.task_gradient_size(0), "actor_P": pc.task_gradient_size(1),
            "finite_logs": bool(all(np.isfinite(v) for k, v in logs.items() if "cosine" not in k)),
        }
        if ca:
            out |= {"cagrad_step": spread(tc), "ratio_cagrad_over_pcgrad": statistics.median(tc) / statistics.median(tq)}
            ca.close()
        if gn:
            st = [gn.gradnorm_state(w) for w in range(2)]
            out |= {"gradnorm_step": spread(tg), "ratio_gradnorm_over_cagrad": statistics.median(tg) / statistics.median(tc),
                    "gradnorm_inner_counts": [s.count for s in st],
                    "gradnorm_weights_finite": bool(all(np.all(np.isfinite(s.task_weights)) for s in st))}
            gn.close()
        print(json.dumps(out), flush=True)
        plain.close()
        pc.close()


if __name__ == "__main__":
    main()
