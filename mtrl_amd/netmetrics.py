"""Network health metrics of the MTSAC trunks: dormant-neuron logs and srank.

The device pass (``MTSACEngine.network_metrics``, csrc/netmetrics.hip) leaves, for every trunk layer of every
network member, the normalised neuron scores with their dormant count and the float64 Gram matrix of the
activations.  This module turns them into the reference's LogDict (``MTSAC.get_metrics``, mtsac.py; the key
names of ``get_dormant_neuron_logs`` and ``compute_srank``, mtrl/monitoring/metrics.py).

srank from a Gram matrix: the singular values of ``H`` are the square roots of the eigenvalues of ``H^T H``
(or ``H H^T``, whichever is smaller), so ``numpy.linalg.eigvalsh`` of the r x r float64 Gram replaces the SVD
of the B x W activations.  The Gram is accumulated in float64 from exact products of the float32 activations,
so it resolves what a float32 SVD of ``H`` resolves.

Two points of the reference, pinned by tests/test_network_metrics_cpu.py:

* ``Metrics.is_enabled`` reads ``self.value & other.value == other.value``.  In Python ``&`` binds tighter than
  ``==`` (unlike C), so this is ``(self.value & other.value) == other.value``, a plain flag test: NONE enables
  nothing, DORMANT_NEURONS the dormant logs, SRANK the srank logs, ALL both.  ``network_logs`` calls the enum's
  method as it stands, and the device pass computes only the group that is asked for.
* the reference's ``_get_intermediates`` passes ``task_ids`` to networks that take none and reads a
  ``VmapBRCCritic_0`` key the multi-head critic does not have, so it cannot run on these networks; what is
  computed here is its evident intent (the ``torso_layer_{i}`` post-ReLU outputs of actor and online critic).
"""

from __future__ import annotations

import numpy as np

DORMANT_THRESHOLD = 0.1  # get_dormant_neuron_logs' default
SRANK_DELTA = 0.01       # compute_srank's default


def srank_from_singular_values(sigma, delta: float = SRANK_DELTA) -> int:
    """The smallest k (1-based) with cumsum(sigma)_k / sum(sigma) >= 1 - delta, sigma descending.  All-zero
    sigma: every ratio is NaN, every comparison false, argmax of all-false is 0 -> srank 1."""
    s = np.sort(np.asarray(sigma, np.float64))[::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = np.cumsum(s) / np.sum(s)
    return int(np.argmax(ratios >= 1.0 - delta)) + 1


def singular_values_from_gram(gram) -> np.ndarray:
    """sigma (descending) of H from its float64 Gram matrix: sqrt(max(lambda, 0))."""
    lam = np.linalg.eigvalsh(np.asarray(gram, np.float64))
    return np.sqrt(np.maximum(lam, 0.0))[::-1]


def singular_values_from_eigvals(lam) -> np.ndarray:
    """sigma (descending) from the Gram's eigenvalues in ascending order (the device solve)."""
    return np.sqrt(np.maximum(np.asarray(lam, np.float64), 0.0))[::-1]


def srank_from_gram(gram, delta: float = SRANK_DELTA) -> int:
    return srank_from_singular_values(singular_values_from_gram(gram), delta)


def dormant_logs(counts, width: int) -> dict:
    """get_dormant_neuron_logs' entries of one member from its per-layer dormant counts [D]."""
    counts = [int(c) for c in counts]
    logs = {}
    for i, c in enumerate(counts):
        logs[f"torso_layer_{i}_ratio"] = c / width * 100
        logs[f"torso_layer_{i}_count"] = c
    total = sum(counts)
    logs["total_ratio"] = total / (len(counts) * width) * 100
    logs["total_count"] = total
    return logs


def member_names(num_critics: int) -> list[str]:
    return ["actor"] + [f"critic_{e}" for e in range(num_critics)]


def network_logs(metrics, members: dict) -> dict:
    """The LogDict of ``MTSAC.get_metrics``.  ``metrics``: a ``compat.config.utils.Metrics`` member (its
    ``is_enabled`` decides).  ``members``: name ("actor", "critic_0", ...) ->
    ``{"width": W, "counts": [D] or None, "srank": [D] or None}`` in the reference's order."""
    from .compat.config.utils import Metrics

    logs = {}
    for name, m in members.items():
        if metrics.is_enabled(Metrics.DORMANT_NEURONS):
            logs.update({f"metrics/dormant_neurons_{name}_{k}": v
                         for k, v in dormant_logs(m["counts"], m["width"]).items()})
        if metrics.is_enabled(Metrics.SRANK):
            for i, k in enumerate(m["srank"]):
                logs[f"metrics/srank_{name}_torso_layer_{i}"] = int(k)
    return logs


def expected_keys(depth_actor: int, depth_critic: int, num_critics: int) -> list[str]:
    """Every key of a full (both groups) LogDict."""
    keys = []
    for name, D in [("actor", depth_actor)] + [(f"critic_{e}", depth_critic) for e in range(num_critics)]:
        for i in range(D):
            keys += [f"metrics/dormant_neurons_{name}_torso_layer_{i}_ratio",
                     f"metrics/dormant_neurons_{name}_torso_layer_{i}_count"]
        keys += [f"metrics/dormant_neurons_{name}_total_ratio", f"metrics/dormant_neurons_{name}_total_count"]
        keys += [f"metrics/srank_{name}_torso_layer_{i}" for i in range(D)]
    return keys


def _sranks(r, e) -> list[int]:
    """srank of every layer of member e from one network's ``network_metrics`` result (either eig path)."""
    if r["gram"] is None:
        return [srank_from_singular_values(singular_values_from_eigvals(lam)) for lam in r["eigvals"][e]]
    return [srank_from_gram(g) for g in r["gram"][e]]


def compute_metrics(engine, metrics, observations=None, eps=None, threshold: float = DORMANT_THRESHOLD,
                    eig: str = "host") -> dict:
    """One device pass on ``engine`` and the LogDict.  Nothing runs when ``metrics`` enables neither group.
    ``eig``: where the Grams' eigenvalues are computed, "host" (``numpy.linalg.eigvalsh`` on copies of the Grams)
    or "device" (the engine's Householder + bisection solve; raises on a non-finite Gram)."""
    from .compat.config.utils import Metrics

    dormant = bool(metrics.is_enabled(Metrics.DORMANT_NEURONS))
    srank = bool(metrics.is_enabled(Metrics.SRANK))
    if not (dormant or srank):
        return {}
    if eig not in ("host", "device"):
        raise ValueError(f"eig must be 'host' or 'device', not {eig!r}")
    if eig == "device" and srank:
        out = engine.network_metrics(observations, eps, dormant=dormant, gram=True, threshold=threshold, eig="device")
        for net in ("actor", "critic"):
            if np.any(out[net]["eig_flags"]):
                raise FloatingPointError(f"non-finite activation Gram in the {net} trunk (flags "
                                         f"{out[net]['eig_flags'].tolist()}): no srank")
    else:  # the call the host path has always made
        out = engine.network_metrics(observations, eps, dormant=dormant, gram=srank, threshold=threshold)
    members = {}
    for which, net in enumerate(("actor", "critic")):
        r = out[net]
        for e in range(r["members"]):
            name = "actor" if which == 0 else f"critic_{e}"
            members[name] = {"width": r["width"],
                             "counts": r["counts"][e] if dormant else None,
                             "srank": _sranks(r, e) if srank else None}
    return network_logs(metrics, members)
