"""Per-task batch-size samplers (mtrl/rl/sampling_algs.py), in numpy.

The reference module does not import (it uses ``jnp`` without importing it), so these classes are written
from its formulas, keeping what the formulas do at the edges:

* ``Sampler``: sizes proportional to the losses, ``(loss / sum(loss) * B).astype(int)`` -- truncation toward
  zero -- and the remainder ``B - sum(sizes)`` handed out one row each to the FIRST ``remainder`` tasks
  (``batch_sizes[:remainder] += 1``), whatever their losses.
* ``AdaptiveSampler``: an EMA of the losses (from ones, float32 as ``jnp.ones``), a softmax with temperature
  (``exp(l) / sum(exp(l))``, no max subtraction), the same truncation, and the remainder to the
  ``remainder`` tasks of highest weight (the tail of a stable ascending argsort, so ties go to the later tasks).

Both return ``int64`` sizes that sum to ``total_batch_size`` for finite positive losses: each truncation
loses less than one row, so the remainder lies in [0, T).
"""

from __future__ import annotations

import numpy as np


class AdaptiveSampler:
    def __init__(self, n_tasks: int, ema_alpha: float = 0.1, temperature: float = 1.0):
        self.n_tasks = n_tasks
        self.ema_alpha = ema_alpha
        self.temperature = temperature
        self.task_losses_ema = np.ones(n_tasks, np.float32)

    def update(self, task_losses) -> None:
        losses = np.asarray(task_losses, np.float32)
        self.task_losses_ema = (np.float32(self.ema_alpha) * losses
                                + np.float32(1 - self.ema_alpha) * self.task_losses_ema).astype(np.float32)

    def get_sampling_weights(self) -> np.ndarray:
        logits = self.task_losses_ema / np.float32(self.temperature)
        e = np.exp(logits)
        return (e / e.sum()).astype(np.float32)

    def sample_batch_sizes(self, task_losses, total_batch_size: int) -> np.ndarray:
        self.update(task_losses)
        weights = self.get_sampling_weights()
        batch_sizes = (weights * np.float32(total_batch_size)).astype(int)
        remainder = int(total_batch_size - batch_sizes.sum())
        if remainder > 0:
            top_indices = np.argsort(weights, kind="stable")[-remainder:]
            batch_sizes[top_indices] += 1
        return batch_sizes


class Sampler:
    def sample_batch_sizes(self, task_losses, total_batch_size: int) -> np.ndarray:
        task_losses = np.asarray(task_losses)
        loss_weights = task_losses / task_losses.sum()
        batch_sizes = (loss_weights * total_batch_size).astype(int)
        remainder = int(total_batch_size - batch_sizes.sum())
        batch_sizes[:remainder] += 1
        return batch_sizes


def make_sampler(sampler_type: str | None, num_tasks: int):
    """``TrainingConfig.sampler_type``: None (no sampler), "loss" (Sampler) or "adaptive" (AdaptiveSampler)."""
    if sampler_type is None:
        return None
    if sampler_type == "loss":
        return Sampler()
    if sampler_type == "adaptive":
        return AdaptiveSampler(num_tasks)
    raise ValueError(f'sampler_type must be None, "loss" or "adaptive", got {sampler_type!r}')
