"""OptimizerConfig (mtrl/config/optim.py:14-43): optax.chain(clip_by_global_norm, adam(eps=1e-5))
is executed by the engine's optimizer kernels (mtrl_amd/csrc/optim.hip)."""

from dataclasses import dataclass
from typing import Any

from .utils import Optimizer


@dataclass(frozen=True, kw_only=True)
class OptimizerConfig:
    lr: float = 3e-4
    optimizer: Optimizer = Optimizer.Adam
    max_grad_norm: float | None = None
    eps: float | None = None
    weight_decay: float | None = None

    @property
    def requires_split_task_losses(self) -> bool:
        return False

    @property
    def adam_eps(self) -> float:  # config/optim.py:29-32
        return self.eps if self.eps is not None else 1e-5


@dataclass(frozen=True, kw_only=True)
class PCGradConfig(OptimizerConfig):
    """config/optim.py:59-72: optax.chain(pcgrad(num_tasks, cosine_sim_logs), clip, adam).  The engine
    runs the surgery in Gram form on the per-task gradients (mtrl_amd/csrc/pcgrad.hip); both the actor's
    and the critic's optimizer must be PCGrad (the only combination the reference itself can run)."""

    num_tasks: int
    cosine_sim_logs: bool = False

    @property
    def requires_split_task_losses(self) -> bool:
        return True


@dataclass(frozen=True, kw_only=True)
class CAGradConfig(OptimizerConfig):
    """config/optim.py:100-118: optax.chain(cagrad(num_tasks), clip, adam).  ``cagrad()`` is called with
    its defaults (c = 0.5, 21 iterations, learning rate 25 below 50 tasks and 50 from there on, momentum
    0.5, no cosine logs); ``cagrad_optimizer`` and ``initial_weights`` are fields the reference never
    reads.  The engine runs the weight search in Gram form on the per-task gradients
    (mtrl_amd/csrc/cagrad.hip); both the actor's and the critic's optimizer must be CAGrad."""

    num_tasks: int
    cagrad_optimizer: OptimizerConfig
    initial_weights: Any | None = None
    max_grad_norm: float | None = None

    @property
    def requires_split_task_losses(self) -> bool:
        return True


@dataclass(frozen=True, kw_only=True)
class GradNormConfig(OptimizerConfig):
    """config/optim.py:75-98: optax.chain(gradnorm(num_tasks, gradnorm_optimizer, asymmetry,
    initial_weights, max_grad_norm), clip, adam).  ``gradnorm_optimizer`` is the inner optimizer of the T
    task weights; a truthy ``max_grad_norm`` also clips every task gradient to norm 1.0 (not to
    max_grad_norm: clip_per_task_grads is called with its default bound).  The engine runs the weight step
    in Gram form on the per-task gradients and losses (mtrl_amd/csrc/gradnorm.hip); both the actor's and
    the critic's optimizer must be GradNorm."""

    num_tasks: int
    gradnorm_optimizer: OptimizerConfig
    initial_weights: Any | None = None
    asymmetry: float = 0.12
    max_grad_norm: float | None = None

    @property
    def requires_split_task_losses(self) -> bool:
        return True
