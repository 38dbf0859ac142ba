"""Per-element allowance for a gradient leaf of the plain MTSAC step against the float64 oracle.

Every parameter gradient is the last product of the backward pass: a kernel's is in^T dz, a hidden
bias's the column sums of dz, a head's the same with the head's dout.  The project's GEMMs promise
|error| <= 4e-6 sum |a| |b| (include/mtsac.h), and the tests allow 1e-5 mag per element: 2.5 times the
bound of the GEMM that produces the leaf, the rest for its operands, which upstream GEMMs rounded.

What `mag` has to be.  The plain product on absolute values, |in|^T |dz|, bounds the last GEMM's own
error only.  Its operands carry errors that are not proportional to their own size: a hidden
activation in = relu(x W + b) that comes out at 1e-3 from terms of size 1 is wrong by 1e-7 of those
terms, 1e-4 of itself, and dz = (dz_up W^T) mask cancels the same way.  With 2-5 rows per task a
kernel element is often one such product, and the float32 oracle itself then misses 1e-5 |in|^T |dz| by
a factor 5 (test_adam_ref_cpu.test_float32_oracle_meets_the_leaf_allowance measured up to 5.9e-5).  So
`mag` carries the magnitudes along both passes:

    F_0 = |x|,  F_{i+1} = F_i |W_i| + |b_i|                 (>= |h_{i+1}|, the forward's absolute terms)
    D_top = |dout| |Wh|^T,  D_i = mask_i (D_{i+1} |W_{i+1}|^T)   (>= |dz_i|, the backward's)
    kernel i: F_i^T D_i    bias i: column sums of D_i    head: F_depth (x) |dout|, |dout|

An error of k roundings in an operand is then k 2^-24 of F or D, far inside the share 6e-6 mag left
for it.  The plain product is returned as well (`plain`), and the GPU test prints the ratio against it.

`update_with_magnitudes` runs oracle.mtsac.update and returns, beside its results, both magnitudes for
the critic and the actor in the flat leaf order of the gradients."""

from __future__ import annotations

import numpy as np

from oracle import mtsac as om

GRAD_RTOL = 1e-5


def backward_magnitudes(p: dict, hs, t, dout, depth: int):
    """(mag, plain) of om.mh_backward's products, with the masks of the true passes."""
    m = {k: np.zeros_like(v) for k, v in p.items()}
    q = {k: np.zeros_like(v) for k, v in p.items()}
    F = [np.abs(hs[0])]
    for i in range(depth):
        F.append(F[i] @ np.abs(p[f"W{i}"]) + np.abs(p[f"b{i}"]))
    ad = np.abs(dout)
    np.add.at(m["head_W"], t, np.einsum("bw,bo->bwo", F[depth], ad))
    np.add.at(q["head_W"], t, np.einsum("bw,bo->bwo", np.abs(hs[depth]), ad))
    np.add.at(m["head_b"], t, ad)
    np.add.at(q["head_b"], t, ad)
    dh = np.einsum("bo,bwo->bw", dout, p["head_W"][t])
    D = np.einsum("bo,bwo->bw", ad, np.abs(p["head_W"][t]))
    for i in reversed(range(depth)):
        mask = hs[i + 1] > 0
        dz, D = dh * mask, D * mask
        m[f"W{i}"], q[f"W{i}"] = F[i].T @ D, np.abs(hs[i]).T @ np.abs(dz)
        m[f"b{i}"], q[f"b{i}"] = D.sum(axis=0), np.abs(dz).sum(axis=0)
        if i > 0:
            dh, D = dz @ p[f"W{i}"].T, D @ np.abs(p[f"W{i}"]).T
    return m, q


def update_with_magnitudes(cfg: om.OracleConfig, state: om.MTSACState, batch, eps_next, eps_cur):
    """(new_state, logs, internals, mags) of one oracle step; mags = {"critic": (mag, plain), "actor": ...}.

    om.update calls mh_backward once per critic member for the critic's gradient, once per member with
    need_dx for the actor's pass through the critic (no parameter gradient: skipped) and once for the
    actor; the calls are recorded through a wrapper so the magnitudes use the very dout of the step."""
    calls = []
    real = om.mh_backward

    def recording(p, hs, t, dout, depth, need_dx=False):
        if not need_dx:
            calls.append(backward_magnitudes(p, hs, t, dout, depth))
        return real(p, hs, t, dout, depth, need_dx)

    om.mh_backward = recording
    try:
        new, logs, internals = om.update(cfg, state, batch, eps_next, eps_cur, return_internals=True)
    finally:
        om.mh_backward = real
    C = cfg.num_critics
    assert len(calls) == C + 1
    csh, ash = om.critic_leaf_shapes(cfg), om.actor_leaf_shapes(cfg)
    mags = {"critic": tuple(om.flatten({k: np.stack([calls[e][j][k] for e in range(C)]) for k, _ in csh}, csh)
                            for j in (0, 1)),
            "actor": tuple(om.flatten(calls[C][j], ash) for j in (0, 1))}
    return new, logs, internals, mags


def leaf_report(got, want, mag, shapes):
    """[(leaf name, max |got - want| / mag over the leaf's elements with mag > 0, exact where mag == 0)]."""
    out, o = [], 0
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for name, s in shapes:
        n = int(np.prod(s))
        d, m = np.abs(got[o:o + n] - want[o:o + n]), mag[o:o + n]
        nz = m > 0
        out.append((name, float(np.max(d[nz] / m[nz])) if nz.any() else 0.0, bool(np.all(d[~nz] == 0))))
        o += n
    return out
