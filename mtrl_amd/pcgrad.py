"""PCGrad gradient surgery (mtrl/optim/pcgrad.py:38-134) in Gram form, numpy float64.

Every projected gradient stays in the span of the task gradients, ``g_i^pc = sum_k C[i][k] g_k``, so
with ``G = M M^T`` the surgery is T x T algebra:

    D[i][:] = g_i^pc . g_:  (= C[i] G)
    step j of row i:  proj = D[i][j] / (G[j][j] + 1e-8)
    proj < 0:         C[i][j] -= proj,  D[i][:] -= proj G[j][:]

and the update handed to the rest of the optimizer chain is ``mean_i g_i^pc = sum_k w_k g_k`` with
``w = mean_i C[i]``.  ``pcgrad_from_gram`` is the host statement of the device solve
(csrc/pcgrad.hip); ``pcgrad_direct`` is the reference's literal sequential projection, kept to pin it.
"""

from __future__ import annotations

import numpy as np

LOG_KEYS = ("n_grad_conflicts", "avg_grad_magnitude", "avg_grad_magnitude_before_surgery",
            "avg_cosine_similarity", "avg_cosine_similarity_diff")


def _avg_cos(F: np.ndarray) -> float:
    """vmap_cos_sim of pcgrad.py:97-121 from a Gram matrix: mean over the upper triangle of
    F_ij / (|g_i| |g_j| + 1e-8)."""
    T = F.shape[0]
    nrm = np.sqrt(np.maximum(np.diag(F), 0.0))
    cos = F / (nrm[:, None] * nrm[None, :] + 1e-8)
    return float(np.triu(cos, k=1).sum() / (T * (T - 1) / 2 + 1e-8))


def pcgrad_from_gram(gram, perm=None, cosine_sim_logs: bool = False):
    """(w [T] in original task order, logs) from the Gram matrix of the task gradients.

    ``perm``: the order the tasks are taken in (``jax.random.permutation`` of the rows before
    ``_pcgrad``; default the identity).  ``logs`` holds the five ``PCGradState`` values and
    ``grad_magnitude`` = |mean_t g_t| (what the reference logs as ``*_grad_magnitude``).
    """
    G0 = np.asarray(gram, np.float64)
    T = G0.shape[0]
    perm = np.arange(T) if perm is None else np.asarray(perm, np.int64)
    G = G0[np.ix_(perm, perm)]
    C = np.eye(T)
    D = G.copy()
    conflicts = 0
    for i in range(T):
        for j in range(T):
            proj = D[i, j] / (G[j, j] + 1e-8)
            if proj < 0:
                conflicts += 1
                C[i, j] -= proj
                D[i] -= proj * G[j]
    F = C @ G @ C.T
    w = np.zeros(T)
    w[perm] = C.mean(axis=0)
    logs = {
        "n_grad_conflicts": conflicts / 2,
        "avg_grad_magnitude": float(np.sqrt(np.maximum(np.diag(F), 0.0)).mean()),
        "avg_grad_magnitude_before_surgery": float(np.sqrt(np.maximum(np.diag(G), 0.0)).mean()),
        "avg_cosine_similarity": float("nan"),
        "avg_cosine_similarity_diff": float("nan"),
        "grad_magnitude": float(np.sqrt(max(G.sum(), 0.0)) / T),
    }
    if cosine_sim_logs:
        before = _avg_cos(G)
        logs["avg_cosine_similarity"] = before
        logs["avg_cosine_similarity_diff"] = before - _avg_cos(F)
    return w, logs


def pcgrad_direct(M, perm=None, cosine_sim_logs: bool = False):
    """The reference's sequential projection on the gradients themselves (pcgrad.py:56-95):
    (update [P] = mean_i g_i^pc, logs)."""
    M = np.asarray(M, np.float64)
    T = M.shape[0]
    perm = np.arange(T) if perm is None else np.asarray(perm, np.int64)
    Mp = M[perm]
    final = np.empty_like(Mp)
    conflicts = 0
    for i in range(T):
        g = Mp[i].copy()
        for j in range(T):
            proj = np.dot(g, Mp[j]) / ((Mp[j] ** 2).sum() + 1e-8)
            g = g - min(proj, 0.0) * Mp[j]
            conflicts += int(proj < 0)
        final[i] = g
    logs = {
        "n_grad_conflicts": conflicts / 2,
        "avg_grad_magnitude": float(np.linalg.norm(final, axis=1).mean()),
        "avg_grad_magnitude_before_surgery": float(np.linalg.norm(Mp, axis=1).mean()),
        "avg_cosine_similarity": float("nan"),
        "avg_cosine_similarity_diff": float("nan"),
        "grad_magnitude": float(np.linalg.norm(Mp.mean(axis=0))),
    }
    if cosine_sim_logs:
        before = _avg_cos(Mp @ Mp.T)
        logs["avg_cosine_similarity"] = before
        logs["avg_cosine_similarity_diff"] = before - _avg_cos(final @ final.T)
    return final.mean(axis=0), logs
