"""Float64 statements of the network health metrics (dormant neurons, srank) and the error bars of the engine's
pass against them.  Nothing here looks at a kernel's output.  Shared by tests/test_network_metrics_cpu.py and
tests/test_gpu_network_metrics.py.

Statements (reference get_dormant_neuron_logs / compute_srank, mtrl/monitoring/metrics.py), for H [B][W]:
    s_j = mean_b |H[b][j]|,  s~_j = s_j / (mean_j s_j + 1e-9),  dormant: s~_j <= 0.1
    srank = the smallest k (1-based) with cumsum(sigma)_k / sum(sigma) >= 0.99, sigma = svd(H) descending;
    an all-zero H gives NaN ratios, all comparisons false, argmax 0 -> srank 1.

Bars of the whole path: the engine's trunk GEMMs are documented (include/mtsac.h, enum mtsac_precision) to
|error| <= GEMM_BOUND * sum_k |a_k b_k| per output at every precision.  `forward_with_bounds` carries that through
the float64 forward layer by layer (ReLU is 1-Lipschitz; the error of a layer's input passes through |W|), and
through the policy head and the tanh-normal sample into the critic's action columns with float32 rounding bars.
"""

from __future__ import annotations

import numpy as np

from oracle import mtsac as om

U = 2.0 ** -24          # float32 unit roundoff
GEMM_BOUND = 4e-6       # include/mtsac.h: the trunk GEMMs' |error| <= 4e-6 sum |a b|
THRESHOLD = 0.1
LIBM = 4                # ulps granted to expf / tanhf


# ------------------------------------------------------------------ statements
def scores(H):
    """(s, s~) of H [B][W] in float64."""
    s = np.mean(np.abs(np.asarray(H, np.float64)), axis=0)
    return s, s / (np.mean(s) + 1e-9)


def dormant_count(H, threshold=THRESHOLD) -> int:
    return int(np.sum(scores(H)[1] <= threshold))


def srank_svd(H, delta=0.01) -> int:
    """The literal statement: SVD of H in float64."""
    s = np.linalg.svd(np.asarray(H, np.float64), compute_uv=False)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = np.cumsum(s) / np.sum(s)
    return int(np.argmax(ratios >= 1.0 - delta)) + 1


def gram64(H):
    """H^T H (W <= M) or H H^T (W > M) in float64, and which side (0 / 1)."""
    H = np.asarray(H, np.float64)
    M, W = H.shape
    return (H.T @ H, 0) if W <= M else (H @ H.T, 1)


def member_logs(name, layers, threshold=THRESHOLD) -> dict:
    """All log entries of one member from its list of layer activations (float64 statements)."""
    logs, total, hidden = {}, 0, 0
    for i, H in enumerate(layers):
        c, W = dormant_count(H, threshold), H.shape[1]
        logs[f"metrics/dormant_neurons_{name}_torso_layer_{i}_ratio"] = c / W * 100
        logs[f"metrics/dormant_neurons_{name}_torso_layer_{i}_count"] = c
        logs[f"metrics/srank_{name}_torso_layer_{i}"] = srank_svd(H)
        total, hidden = total + c, hidden + W
    logs[f"metrics/dormant_neurons_{name}_total_ratio"] = total / hidden * 100
    logs[f"metrics/dormant_neurons_{name}_total_count"] = total
    return logs


# ------------------------------------------------------------------ the whole path with its bars
def _trunk(p, x, ex, depth):
    """Post-ReLU outputs h_i of the trunk on x and the bars e_i of the engine's h_i: the input's bar through
    |W|, plus the GEMM bound on the products of the (perturbed) input, plus the bias add's rounding."""
    hs, es, fs = [], [], []
    h, e = x, ex
    f = float(np.sqrt(np.sum(ex * ex)))
    for i in range(depth):
        W, b = p[f"W{i}"], p[f"b{i}"]
        z = h @ W + b
        S = (np.abs(h) + e) @ np.abs(W)
        fresh = GEMM_BOUND * S
        e = e @ np.abs(W) + fresh
        round_ = 2 * U * (np.abs(z) + e)  # the epilogue's float32 bias add
        e = e + round_
        dead = z + e <= 0  # certainly non-positive before the ReLU: exactly zero on both sides
        e = np.where(dead, 0.0, e)
        # the same error in the Frobenius norm: |dH_i|_F <= |dH_{i-1}|_F |W|_2 + |fresh + rounding|_F
        f = f * np.linalg.norm(W, 2) + float(np.sqrt(np.sum(np.where(dead, 0.0, fresh + round_) ** 2)))
        f = min(f, float(np.sqrt(np.sum(e * e))))
        h = np.maximum(z, 0)
        hs.append(h)
        es.append(e)
        fs.append(f)
    return hs, es, fs


def forward_with_bounds(cfg, actor_flat, critic_flat, obs, eps):
    """Float64 forward of get_metrics' pass (actor on obs, a = tanh(mu + sigma eps), online critic on (a, obs))
    and the bars of the engine's activations.  Returns {member: [(H, E, F) per layer]}: E elementwise, F on the
    Frobenius norm of the difference."""
    A, T = cfg.action_dim, cfg.num_tasks
    obs, eps = np.asarray(obs, np.float64), np.asarray(eps, np.float64)
    pa = om.unflatten(np.asarray(actor_flat, np.float64), om.actor_leaf_shapes(cfg))
    pc = om.unflatten(np.asarray(critic_flat, np.float64), om.critic_leaf_shapes(cfg))
    out, hs_o, t = om.mh_forward(pa, obs, cfg.actor_depth, T)
    a, _, _ = om.tanh_normal_sample(out, eps, cfg)
    hs, es, fs = _trunk(pa, obs, np.zeros_like(obs), cfg.actor_depth)
    assert all(np.array_equal(x, y) for x, y in zip(hs, hs_o[1:]))
    members = {"actor": list(zip(hs, es, fs))}
    # policy head (a float32 dot over W terms, any order: <= (W + 2) U sum |terms|) and the tanh-normal tail
    h, e = hs[-1], es[-1]
    Wh, bh = np.abs(pa["head_W"][t]), np.abs(pa["head_b"][t])
    S_out = np.einsum("bw,bwo->bo", np.abs(h) + e, Wh) + bh
    e_out = np.einsum("bw,bwo->bo", e, Wh) + (cfg.actor_width + 2) * U * S_out
    mu, ls = out[:, :A], out[:, A:]
    sigma = np.exp(np.clip(ls, cfg.log_std_min, cfg.log_std_max))
    e_sigma = sigma * (np.expm1(e_out[:, A:]) + LIBM * U)
    e_x = e_out[:, :A] + np.abs(eps) * e_sigma + 2 * U * (np.abs(mu) + np.abs(sigma * eps))
    e_a = e_x + LIBM * U  # |tanh'| <= 1, |a| <= 1
    x = np.concatenate([a, obs], axis=1)
    ex = np.concatenate([e_a, np.zeros_like(obs)], axis=1)
    _, caches = om.critic_forward(pc, x, cfg)
    for k in range(cfg.num_critics):
        hs, es, fs = _trunk(om.ens_slice(pc, k), x, ex, cfg.critic_depth)
        assert all(np.array_equal(u, v) for u, v in zip(hs, caches[k][0][1:]))
        members[f"critic_{k}"] = list(zip(hs, es, fs))
    return members


def score_bound(H, E):
    """Bar of the engine's normalised scores: the activations' bar through the two means and the quotient,
    plus the float32 roundings of s, the denominator and the quotient."""
    s, sn = scores(H)
    e_s = np.mean(E, axis=0) + U * s
    den = np.mean(s) + 1e-9
    e_den = np.mean(e_s) + U * den
    return e_s / (den - e_den) + s * e_den / (den * (den - e_den)) + 2 * U * sn


def srank_margin(H, eps):
    """(srank, ok, gap, need): the reference's ratio at k* and k* - 1 must lie farther from 0.99 than
    need = 2 r eps / (total - r eps), eps >= |dH|_F >= |dH|_2 >= every singular value's shift (Weyl)."""
    s = np.linalg.svd(np.asarray(H, np.float64), compute_uv=False)
    r, total = s.size, float(np.sum(s))
    k = srank_svd(H)
    if total == 0.0:
        return k, eps == 0.0, np.inf, 0.0
    need = 2 * r * eps / (total - r * eps) if total > r * eps else np.inf
    ratios = np.cumsum(s) / total
    gap = min(abs(ratios[j] - 0.99) for j in (k - 1, k - 2) if j >= 0)
    return k, gap > need, gap, need


# ------------------------------------------------------------------ the whole-path cases
# (T, n, W, D, A, E) -> (seed, protos) for which the float64 reference alone meets both margin conditions (found
# on the CPU with `qualifying_seed`; every test asserts them again).  Where the activations have full rank the
# ratio curve climbs by about 1 / r per singular value near the 99 % mark, and at r = 130 no seed leaves the
# margin 2 r eps / (total - r eps) the documented GEMM bound asks for (seeds 0 .. 39 searched); the wide case
# therefore runs on a collapsed batch (make_case: protos), the regime the metric is watched for.
WHOLE_CASES = {
    (3, 5, 36, 3, 4, 2): (3, None),
    (10, 13, 132, 2, 6, 1): (1, 2),
    (2, 17, 20, 1, 1, 3): (0, None),
}


def make_case(shape, seed, protos=None):
    """Config, float32-exact parameters (flat, flax order), observations and eps of one whole-path case.  Planted
    negative biases kill some neurons of every layer (dead for every row: exactly zero activations).  protos: a
    task's rows repeat that many distinct (observation, eps) rows -- a collapsed batch whose activations have rank
    <= T * protos, so that the 99 % mark falls on the steep part of the spectrum."""
    T, n, W, D, A, E = shape
    cfg = om.OracleConfig(num_tasks=T, obs_dim=39 + T, action_dim=A, actor_width=W, actor_depth=D, critic_width=W,
                          critic_depth=D, num_critics=E)
    st = om.initialize(cfg, seed=100 + seed)
    rng = np.random.default_rng(7000 + seed)
    pa = om.unflatten(st.actor, om.actor_leaf_shapes(cfg))
    pc = om.unflatten(st.critic, om.critic_leaf_shapes(cfg))
    for i in range(D):
        pa[f"b{i}"] = rng.uniform(-0.1, 0.1, W)
        pa[f"b{i}"][rng.choice(W, max(1, W // 7), replace=False)] = -50.0
        pc[f"b{i}"] = rng.uniform(-0.1, 0.1, (E, W))
        for k in range(E):
            pc[f"b{i}"][k, rng.choice(W, max(1, W // 9 + k), replace=False)] = -50.0
    actor = om.flatten(pa, om.actor_leaf_shapes(cfg)).astype(np.float32)
    critic = om.flatten(pc, om.critic_leaf_shapes(cfg)).astype(np.float32)
    B = n * T
    t = np.arange(B) % T
    obs = np.zeros((B, 39 + T), np.float32)
    obs[:, :39] = rng.standard_normal((B, 39))
    obs[np.arange(B), 39 + t] = 1.0
    eps = rng.standard_normal((B, A)).astype(np.float32)
    if protos:  # row i*T + t repeats row (i % protos)*T + t
        src = (np.arange(B) // T % protos) * T + t
        obs, eps = obs[src], eps[src]
    return cfg, actor, critic, obs, eps


def case_expectations(shape, seed, protos=None):
    """Per member and layer: the float64 (s~, bar, count, srank) and whether the margin conditions hold."""
    cfg, actor, critic, obs, eps = make_case(shape, seed, protos)
    members = forward_with_bounds(cfg, actor, critic, obs, eps)
    exp, ok = {}, True
    for name, layers in members.items():
        rows = []
        for H, E, F in layers:
            _, sn = scores(H)
            bar = score_bound(H, E)
            near = bool(np.any(np.abs(sn - THRESHOLD) <= bar))
            k, sr_ok, gap, need = srank_margin(H, F)
            ok = ok and not near and sr_ok
            rows.append(dict(norm=sn, bar=bar, count=int(np.sum(sn <= THRESHOLD)), srank=k, near=near, srank_ok=sr_ok,
                             gap=gap, need=need))
        exp[name] = rows
    return (cfg, actor, critic, obs, eps), exp, ok


def qualifying_seed(shape, protos=None, tries=200):
    for seed in range(tries):
        if case_expectations(shape, seed, protos)[2]:
            return seed
    return None
