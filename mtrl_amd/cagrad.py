"""CAGrad (mtrl/optim/cagrad.py, CAGradConfig of mtrl/config/optim.py) in Gram form, numpy float64.

The optimizer's whole effect on the per-task gradients ``M`` [T][P] is a vector of T combine weights
computed from ``G = M M^T``:

    clip to norm 1:  s_t = min(1, 1 / (|g_t| + 1e-8)),  G' = diag(s) G diag(s)     (M is never rescaled)
    scaling:         scale = mean_t sqrt(G'_tt + 1e-4),  GG = G' / scale^2,
                     Gg = row means of GG,  gg = mean(Gg),  c_n = c sqrt(gg + 1e-4)
    weight search:   num_iterations - 1 momentum-SGD steps on
                     obj(w) = ww.Gg + c_n sqrt(ww^T GG ww + 1e-4),  ww = w / (sum w + 1e-8),
                     from w = 0, keeping the iterate of the (strictly) lowest objective, plus a final
                     evaluation;  task_weights = softmax(w_best)
    combine:         lambda = c_n / (sqrt(tw^T GG tw + 1e-4) + 1e-4),
                     update = sum_t w_t g_t,  w_t = s_t (1/T + tw_t lambda) / (1 + c^2)

``cagrad_from_gram`` is the host statement of the device solve (csrc/cagrad.hip); ``cagrad_direct`` is
the reference's literal statement on the gradients themselves, with the objective's gradient taken by
``torch.autograd`` in float64, kept to pin the analytic gradient used here and on the device.
"""

from __future__ import annotations

import numpy as np

LOG_KEYS = ("task_weights", "avg_grad_magnitude", "avg_grad_magnitude_before_surgery",
            "avg_cosine_similarity", "cagrad_objective")


def default_learning_rate(num_tasks: int) -> float:
    """cagrad.py:38-39."""
    return 25.0 if num_tasks < 50 else 50.0


def clip_scales(gram) -> np.ndarray:
    """s_t = min(1, 1 / (|g_t| + 1e-8)) from the diagonal of the Gram matrix (cagrad.py:181-184)."""
    nrm = np.sqrt(np.maximum(np.diag(np.asarray(gram, np.float64)), 0.0))
    return np.minimum(1.0, 1.0 / (nrm + 1e-8))


def objective_and_grad(w, GG, Gg, c_n):
    """obj(w) and its analytic gradient: with S = sum w + 1e-8, ww = w / S, q = ww^T GG ww + 1e-4,
    u = Gg + c_n GG ww / sqrt(q):  grad = (u - (ww.u) 1) / S."""
    S = w.sum() + 1e-8
    ww = w / S
    Gw = GG @ ww
    rq = np.sqrt(ww @ Gw + 1e-4)
    obj = ww @ Gg + c_n * rq
    u = Gg + c_n * Gw / rq
    return float(obj), (u - ww @ u) / S


def _softmax(x):
    e = np.exp(x - x.max())
    return e / e.sum()


def _avg_cos(F: np.ndarray) -> float:
    T = F.shape[0]
    nrm = np.sqrt(np.maximum(np.diag(F), 0.0))
    cos = F / (nrm[:, None] * nrm[None, :] + 1e-8)
    return float(np.triu(cos, k=1).sum() / (T * (T - 1) / 2 + 1e-8))


def _search(objective, T, num_iterations, learning_rate, momentum, w0):
    """cagrad.py:83-117: (w_best, obj_best, obj_hist, best_iteration)."""
    w = np.zeros(T) if w0 is None else np.array(w0, np.float64).reshape(T)
    v = np.zeros(T)
    w_best, obj_best, best_it = w.copy(), np.inf, -1
    hist = np.empty(num_iterations)
    for it in range(num_iterations):
        obj, grad = objective(w)
        hist[it] = obj
        if obj < obj_best:
            w_best, obj_best, best_it = w.copy(), obj, it
        if it + 1 < num_iterations:
            v = momentum * v + grad
            w = w - learning_rate * v
    return w_best, obj_best, hist, best_it


def cagrad_from_gram(gram, c: float = 0.5, num_iterations: int = 21, learning_rate: float | None = None,
                     momentum: float = 0.5, w0=None, cosine_sim_logs: bool = False):
    """(w_combine [T] on the raw rows, logs) from the Gram matrix of the raw task gradients.

    ``logs`` holds the five ``CAGradState`` fields, ``grad_magnitude`` = |mean_t g_t| of the raw
    gradients, ``obj_hist`` [num_iterations] (the objective at every evaluated iterate) and
    ``best_iteration``.  ``w0``: the search's start (the reference's, and the training step's, is 0).
    """
    G = np.asarray(gram, np.float64)
    T = G.shape[0]
    lr = default_learning_rate(T) if learning_rate is None else float(learning_rate)
    s = clip_scales(G)
    Gp = s[:, None] * G * s[None, :]
    scale = np.sqrt(np.diag(Gp) + 1e-4).mean()
    GG = Gp / (scale * scale)
    Gg = GG.mean(axis=1)
    gg = Gg.mean()
    c_n = c * np.sqrt(gg + 1e-4)
    w_best, obj_best, hist, best_it = _search(lambda w: objective_and_grad(w, GG, Gg, c_n), T, num_iterations, lr,
                                              momentum, w0)
    tw = _softmax(w_best)
    gw = np.sqrt(tw @ (GG @ tw) + 1e-4)
    lam = c_n / (gw + 1e-4)
    w = s * (1.0 / T + tw * lam) / (1.0 + c * c)
    logs = {
        "task_weights": tw,
        "avg_grad_magnitude": float(np.sqrt(max(w @ (G @ w), 0.0))),
        "avg_grad_magnitude_before_surgery": float(np.sqrt(np.maximum(np.diag(Gp), 0.0)).mean()),
        "avg_cosine_similarity": _avg_cos(Gp) if cosine_sim_logs else float("nan"),
        "cagrad_objective": float(obj_best),
        "grad_magnitude": float(np.sqrt(max(G.sum(), 0.0)) / T),
        "obj_hist": hist,
        "best_iteration": best_it,
        "c_normalized": float(c_n),
    }
    return w, logs


def cagrad_direct(M, c: float = 0.5, num_iterations: int = 21, learning_rate: float | None = None,
                  momentum: float = 0.5, w0=None, cosine_sim_logs: bool = False):
    """The reference's statement on the gradients themselves (cagrad.py:54-232): rows clipped, the Gram
    of the clipped rows, the objective differentiated by torch.autograd in float64:
    (update [P], logs)."""
    import torch

    M = np.asarray(M, np.float64)
    T = M.shape[0]
    lr = default_learning_rate(T) if learning_rate is None else float(learning_rate)
    nrm = np.linalg.norm(M, axis=1)
    Mc = M * np.minimum(1.0, 1.0 / (nrm + 1e-8))[:, None]
    GG = Mc @ Mc.T
    scale = np.sqrt(np.diag(GG) + 1e-4).mean()
    GG = GG / scale ** 2
    Gg = GG.mean(axis=1, keepdims=True)
    gg = Gg.mean()
    c_n = np.sqrt(gg + 1e-4) * c
    GG_t, Gg_t = torch.from_numpy(GG), torch.from_numpy(Gg)

    def objective(w):
        wt = torch.tensor(w.reshape(T, 1), dtype=torch.float64, requires_grad=True)
        ww = wt / (wt.sum() + 1e-8)
        obj = (ww.T @ Gg_t + c_n * torch.sqrt(ww.T @ GG_t @ ww + 1e-4)).squeeze()
        (g,) = torch.autograd.grad(obj, wt)
        return float(obj.detach()), g.numpy().reshape(T)

    w_best, obj_best, hist, best_it = _search(objective, T, num_iterations, lr, momentum, w0)
    tw = _softmax(w_best)
    gw = np.sqrt(tw.reshape(1, -1) @ GG @ tw.reshape(-1, 1) + 1e-4).item()
    lam = c_n / (gw + 1e-4)
    g = ((1.0 / T + tw * lam).reshape(-1, 1) * Mc).sum(axis=0) / (1 + c ** 2)
    logs = {
        "task_weights": tw,
        "avg_grad_magnitude": float(np.linalg.norm(g)),
        "avg_grad_magnitude_before_surgery": float(np.linalg.norm(Mc, axis=1).mean()),
        "avg_cosine_similarity": _avg_cos(Mc @ Mc.T) if cosine_sim_logs else float("nan"),
        "cagrad_objective": float(obj_best),
        "grad_magnitude": float(np.linalg.norm(M.mean(axis=0))),
        "obj_hist": hist,
        "best_iteration": best_it,
        "c_normalized": float(c_n),
    }
    return g, logs
