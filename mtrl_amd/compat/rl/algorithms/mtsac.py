"""MTSAC on the MI355X engine -- the drop-in for mtrl/rl/algorithms/mtsac.py.

``MTSACConfig`` has the reference's fields (mtsac.py:116-127 + AlgorithmConfig);
``MTSAC.initialize / update / sample_action / eval_action / get_num_params`` keep the
reference's functional signatures (``self, logs = self.update(data)``) while the state
lives in one ``MTSACEngine`` (device memory, mutated in place; methods return ``self``).
Supported: multi-head MLP actor/critic (MultiHeadConfig or VanillaNetworkConfig with
num_tasks from the algorithm config), MSE critic, Adam optimizers -- the north-star path --
PCGrad gradient surgery on both networks (PCGradConfig, experiments/misc/mt10_mtmhsac_pcgrad.py) and
CAGrad or GradNorm on both networks (CAGradConfig, experiments/misc/mt10_mtmhsac_cagrad.py; GradNormConfig,
experiments/misc/mt10_mtmhsac_gradnorm.py).  ``MTSAC.initialize(..., shared_head=True)`` (or
MTSAC_VANILLA_SHARED_HEAD=1) runs a VanillaNetworkConfig as the reference builds it: one head shared by all tasks.
"""

from __future__ import annotations

import dataclasses
import os
from collections.abc import Mapping

import numpy as np

from .... import _lib as L
from ....engine import CAGRAD_LOG_KEYS, GRADNORM_LOG_KEYS, PCGRAD_LOG_KEYS, MTSACEngine, make_config
from ....init import init_mtsac, init_vanilla
from ...config.networks import ContinuousActionPolicyConfig, QValueFunctionConfig
from ...config.nn import VanillaNetworkConfig
from ...config.optim import CAGradConfig, GradNormConfig, OptimizerConfig, PCGradConfig
from ...config.rl import AlgorithmConfig
from ...config.utils import Activation, Initializer, Optimizer
from ..buffers import MultiTaskReplayBuffer
from ..sampling_algs import make_sampler
from .base import OffPolicyAlgorithm


@dataclasses.dataclass(frozen=True)
class MTSACConfig(AlgorithmConfig):
    actor_config: ContinuousActionPolicyConfig = ContinuousActionPolicyConfig()
    critic_config: QValueFunctionConfig = QValueFunctionConfig()
    temperature_optimizer_config: OptimizerConfig = OptimizerConfig(max_grad_norm=None)
    initial_temperature: float = 1.0
    num_critics: int = 2
    tau: float = 0.005
    use_task_weights: bool = False
    v_min: float = -10.0
    v_max: float = 10.0
    n_atoms: int = 51


# the engine's gradient-surgery modes (MTSAC.surgery): the fields of the optimizer's state that the reference logs
_SURGERY_LOG_KEYS = {"pcgrad": PCGRAD_LOG_KEYS, "cagrad": CAGRAD_LOG_KEYS, "gradnorm": GRADNORM_LOG_KEYS}


class _DeviceLogs(Mapping):
    """The update's LogDict, fetched from the device on first access (like jax.device_get)."""

    def __init__(self, engine: MTSACEngine, surgery: str | None = None):
        self._engine, self._d, self._surgery = engine, None, surgery

    def _get(self):
        if self._d is None:
            self._d = self._engine.logs()
            if self._surgery:  # the PCGradState / CAGradState / GradNormState fields of both optimizers
                g = getattr(self._engine, f"{self._surgery}_logs")()
                self._d.update({f"metrics/{net}_{k}": g[f"metrics/{net}_{k}"] for net in ("critic", "actor")
                                for k in _SURGERY_LOG_KEYS[self._surgery]})
        return self._d

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(L.LOG_KEYS) + 2 * len(_SURGERY_LOG_KEYS.get(self._surgery, ()))


def _check_supported(net, what: str):
    if getattr(net, "activation", Activation.ReLU) is not Activation.ReLU:
        raise NotImplementedError(f"{what}: only ReLU trunks run on the engine")
    if getattr(net, "kernel_init", Initializer.HE_UNIFORM) is not Initializer.HE_UNIFORM:
        raise NotImplementedError(f"{what}: only he_uniform trunk init is implemented")
    if not getattr(net, "use_bias", True):
        raise NotImplementedError(f"{what}: use_bias=False is not implemented")
    split = net.optimizer.requires_split_task_losses and not isinstance(
        net.optimizer, (PCGradConfig, CAGradConfig, GradNormConfig))
    if net.optimizer.optimizer is not Optimizer.Adam or split:
        raise NotImplementedError(
            f"{what}: only Adam (optax.adam + clip_by_global_norm), plain or behind PCGrad, CAGrad or GradNorm")


def _check_shared_head(net, what: str) -> None:
    """shared_head: the network config must be the reference's plain VanillaNetwork -> MLP (one head layer_D)."""
    if not isinstance(net, VanillaNetworkConfig):
        raise NotImplementedError(
            f"{what}: shared_head runs the VanillaNetworkConfig tree (one Dense head for all tasks); "
            f"{type(net).__name__} has its own heads -- give both networks a VanillaNetworkConfig or leave "
            "shared_head off")
    if net.use_skip_connections:
        raise NotImplementedError(f"{what}: shared_head with use_skip_connections: the engine's trunk has no skip "
                                  "connections")
    if net.use_layer_norm:
        raise NotImplementedError(f"{what}: shared_head with use_layer_norm: the engine's trunk has no layer norm")


def _check_surgery(config: "MTSACConfig", task_shard, config_cls, name: str, one_network: str, sharded: str,
                   tail=None) -> bool:
    """True when both optimizers are ``config_cls``; raises for what the engine's step of that method does not
    run.  ``one_network``, ``sharded``: the method's own reason why the reference / the engine cannot;
    ``tail(opt_a, opt_c)``: its own further checks."""
    opt_a = config.actor_config.network_config.optimizer
    opt_c = config.critic_config.network_config.optimizer
    on_a, on_c = isinstance(opt_a, config_cls), isinstance(opt_c, config_cls)
    if not (on_a or on_c):
        return False
    if on_a != on_c:
        raise NotImplementedError(
            f"{name} on one network only: {one_network}; give both actor and critic a {config_cls.__name__}")
    if opt_a.num_tasks != config.num_tasks or opt_c.num_tasks != config.num_tasks:
        raise ValueError(f"{config_cls.__name__}.num_tasks must equal the algorithm's num_tasks")
    if config.use_task_weights:
        raise NotImplementedError(
            f"{name} with use_task_weights: the reference's split actor loss multiplies by the unsplit closure "
            "variable (mtsac.py:664), which the engine's per-task pass does not reproduce")
    if task_shard is not None:
        raise NotImplementedError(f"{name} on a task-sharded engine: {sharded}")
    if tail:
        tail(opt_a, opt_c)
    return True


def _pcgrad_tail(opt_a, opt_c) -> None:
    if opt_a.cosine_sim_logs != opt_c.cosine_sim_logs:
        raise NotImplementedError("PCGrad: cosine_sim_logs must agree between actor and critic (one engine switch)")


def _gradnorm_tail(opt_a, opt_c) -> None:
    for what, opt in (("actor", opt_a), ("critic", opt_c)):
        inner = opt.gradnorm_optimizer
        if inner.optimizer is not Optimizer.Adam or inner.requires_split_task_losses:
            raise NotImplementedError(f"{what}: GradNormConfig.gradnorm_optimizer must be a plain Adam OptimizerConfig")
        if inner.max_grad_norm is not None and float(inner.max_grad_norm) == 0.0:
            raise ValueError(
                f"{what}: gradnorm_optimizer.max_grad_norm = 0.0: optax.clip_by_global_norm divides the zero "
                "gradient of the task weights by its zero norm (NaN weights in the reference)")
    if opt_a.asymmetry != opt_c.asymmetry:
        raise NotImplementedError("GradNorm: actor and critic asymmetry differ; the engine holds one value")


_SPLIT_ONLY_FOR_ACTOR = ("the reference hands the critic's optimizer per-task gradients only when the ACTOR's "
                         "optimizer asks for split losses (mtsac.py:581), and {}'s shape assert fails on anything else")
# mode -> _check_surgery's arguments: config class, display name, why not on one network, why not sharded, tail
_SURGERY = {
    "pcgrad": (PCGradConfig, "PCGrad",
               "the reference itself cannot run it (mtsac.py:581 averages the critic's per-task gradients unless "
               "the ACTOR's optimizer is PCGrad, and pcgrad's shape assert then fails)",
               "the surgery needs every task's gradient of the whole network on one engine (the Gram matrix "
               "couples all tasks)", _pcgrad_tail),
    "cagrad": (CAGradConfig, "CAGrad", _SPLIT_ONLY_FOR_ACTOR.format("cagrad"),
               "the weight search needs every task's gradient of the whole network on one engine (the Gram matrix "
               "couples all tasks)"),
    "gradnorm": (GradNormConfig, "GradNorm", _SPLIT_ONLY_FOR_ACTOR.format("gradnorm"),
                 "the task weights are renormalised over every task, so all tasks' gradients and losses must be "
                 "on one engine", _gradnorm_tail),
}


def _surgery_mode(config: "MTSACConfig", task_shard) -> str | None:
    """The mode both optimizers ask for (a key of _SURGERY), None for plain Adam."""
    on = [m for m, spec in _SURGERY.items() if _check_surgery(config, task_shard, *spec)]
    return on[0] if on else None


def _switch_on(engine: MTSACEngine, config: "MTSACConfig", mode: str | None, gradnorm_state=()) -> None:
    """The engine's mode on, as the configs ask; ``gradnorm_state``: the (critic, actor) state to carry over."""
    if mode == "pcgrad":
        engine.set_pcgrad(True, config.actor_config.network_config.optimizer.cosine_sim_logs)
    elif mode == "cagrad":
        engine.set_cagrad(True)  # cagrad()'s defaults, as CAGradConfig.spawn calls it
    elif mode == "gradnorm":  # initialised by the switch
        engine.set_gradnorm(True, **_gradnorm_args(config))
        for w, st in enumerate(gradnorm_state):
            engine.set_gradnorm_state(w, st)


def _gradnorm_args(config: "MTSACConfig") -> dict:
    """MTSACEngine.set_gradnorm's arguments from the two GradNormConfigs, (critic, actor) pairs."""
    oc = config.critic_config.network_config.optimizer
    oa = config.actor_config.network_config.optimizer
    iw = None
    if oc.initial_weights is not None or oa.initial_weights is not None:
        T = config.num_tasks
        iw = np.stack([np.ones(T, np.float32) if o.initial_weights is None
                       else np.asarray(o.initial_weights, np.float32).reshape(T) for o in (oc, oa)])
    return dict(asymmetry=oa.asymmetry, per_task_clip=(bool(oc.max_grad_norm), bool(oa.max_grad_norm)),
                inner_lr=(oc.gradnorm_optimizer.lr, oa.gradnorm_optimizer.lr),
                inner_eps=(oc.gradnorm_optimizer.adam_eps, oa.gradnorm_optimizer.adam_eps),
                inner_max_grad_norm=(oc.gradnorm_optimizer.max_grad_norm, oa.gradnorm_optimizer.max_grad_norm),
                initial_weights=iw)


class MTSAC(OffPolicyAlgorithm):
    def __init__(self, config: MTSACConfig, env_config, seed: int, engine: MTSACEngine, cfg_kwargs: dict):
        self.config = config
        self.env_config = env_config
        self.num_tasks = config.num_tasks
        self.engine = engine
        self._cfg_kwargs = cfg_kwargs
        self._rng = np.random.default_rng(seed)  # action noise (replaces jax.random keys, mtsac.py:70-77)
        self._buffer = None  # the replay buffer living in this engine, once spawned
        self.gamma, self.tau = config.gamma, config.tau
        self.target_entropy = -float(np.prod(env_config.action_space.shape))
        # both optimizers PCGrad, CAGrad or GradNorm ("pcgrad", "cagrad", "gradnorm"): the engine runs the
        # gradient-surgery step with that method's solve
        self.surgery: str | None = None
        self.shared_head = False  # the engine holds the Vanilla (shared-head) tree (initialize(shared_head=True))
        # TrainingConfig.sampler_type: the sampler, its period in gradient steps, the steps so far, the sizes in
        # force and every sizes log so far (setup_task_sampler)
        self._sampler = None
        self._sampler_every, self._sampler_steps, self._sampler_sizes = 1, 0, None
        self.sampler_log_history: list[dict] = []

    pcgrad = property(lambda self: self.surgery == "pcgrad")
    cagrad = property(lambda self: self.surgery == "cagrad")
    gradnorm = property(lambda self: self.surgery == "gradnorm")

    # ------------------------------------------------------------------ construction
    @staticmethod
    def initialize(config: MTSACConfig, env_config, seed: int = 1, *, precision: str = "split2h",
                   device: int = 0, task_shard: tuple[int, int] | None = None,
                   shared_head: bool | None = None) -> "MTSAC":
        """task_shard (first task, count): reserved -- this trainer runs unsharded engines (task sharding
        is driven through mtrl_amd.shard).

        shared_head: run a VanillaNetworkConfig as the reference does, VanillaNetwork -> MLP with ONE head
        layer_D shared by all tasks (the engine's MTSAC_NET_SHARED_HEAD), instead of as the multi-head network.
        None reads MTSAC_VANILLA_SHARED_HEAD=1 from the environment; default off, so existing scripts and
        checkpoints keep the multi-head tree.  On, both network configs must be VanillaNetworkConfig without
        skip connections or layer norm (NotImplementedError otherwise)."""
        if shared_head is None:
            shared_head = os.environ.get("MTSAC_VANILLA_SHARED_HEAD") == "1"
        if config.critic_config.use_classification:
            raise NotImplementedError("classification critics are outside the MTSAC MSE path")
        net_a, net_c = config.actor_config.network_config, config.critic_config.network_config
        _check_supported(net_a, "actor")
        _check_supported(net_c, "critic")
        if shared_head:
            _check_shared_head(net_a, "actor")
            _check_shared_head(net_c, "critic")
        surgery = _surgery_mode(config, task_shard)
        if task_shard is not None:
            raise NotImplementedError("task sharding is driven through mtrl_amd.shard, not this trainer")
        T = config.num_tasks
        obs_dim = int(np.prod(env_config.observation_space.shape))
        act_dim = int(np.prod(env_config.action_space.shape))
        kw = dict(
            num_tasks=T, task_count=T, obs_dim=obs_dim, action_dim=act_dim,
            actor_width=net_a.width, actor_depth=net_a.depth, critic_width=net_c.width, critic_depth=net_c.depth,
            num_critics=config.num_critics, gamma=config.gamma, tau=config.tau, clip=int(config.clip),
            use_task_weights=int(config.use_task_weights), actor_lr=net_a.optimizer.lr,
            critic_lr=net_c.optimizer.lr, alpha_lr=config.temperature_optimizer_config.lr,
            actor_max_grad_norm=net_a.optimizer.max_grad_norm, critic_max_grad_norm=net_c.optimizer.max_grad_norm,
            alpha_max_grad_norm=config.temperature_optimizer_config.max_grad_norm,
            adam_eps=net_a.optimizer.adam_eps, initial_temperature=config.initial_temperature,
            log_std_min=config.actor_config.log_std_min, log_std_max=config.actor_config.log_std_max,
            batch_per_task=128, capacity=128, precision=L.PRECISIONS[precision], noise_seed=seed + 1,
        )
        eng = MTSACEngine(make_config(**kw), device=device, shared_head=bool(shared_head))
        _switch_on(eng, config, surgery)
        a, q = (init_vanilla if shared_head else init_mtsac)(T, obs_dim, act_dim, net_a.width, net_a.depth, net_c.width,
                                                             net_c.depth, config.num_critics, seed=seed)
        eng.set_params(L.ACTOR, a)
        eng.set_params(L.CRITIC, q)
        eng.set_params(L.CRITIC_TARGET, q)
        print("Actor Params:", eng.param_count(L.ACTOR))
        print("Critic Params:", eng.param_count(L.CRITIC))
        agent = MTSAC(config, env_config, seed, eng, kw)
        agent.surgery = surgery
        agent.shared_head = bool(shared_head)
        return agent

    def _rebuild(self, **changes) -> None:
        """Re-create the engine with new batch / buffer geometry, keeping parameters, optimizer
        state and the update-noise stream.  Refused once a replay buffer lives in the engine:
        its transitions, pos/full and PCG64 stream would be lost."""
        if self._buffer is not None:
            raise ValueError(f"engine geometry change {changes} after the replay buffer was spawned "
                             "(the device buffer would be lost); keep batch_size fixed for a run")
        keep = {w: self.engine.get_params(w) for w in range(10)}
        counts = [self.engine.get_adam_count(i) for i in range(3)]
        noise = self.engine.noise_state()
        gn_state = [self.engine.gradnorm_state(w) for w in range(2)] if self.gradnorm else []
        self._cfg_kwargs.update(changes)
        old = self.engine
        self.engine = MTSACEngine(make_config(**self._cfg_kwargs), device=old.device, shared_head=self.shared_head)
        old.close()
        _switch_on(self.engine, self.config, self.surgery, gn_state)
        for w, v in keep.items():
            self.engine.set_params(w, v)
        for i, c in enumerate(counts):
            self.engine.set_adam_count(i, c)
        self.engine.set_noise_state(*noise)

    # the reference's MTSAC.key (mtsac.py:134) drives both the update and the action noise; here
    # the update noise is the engine's counter stream and the action noise a numpy Generator
    def noise_key(self) -> np.ndarray:
        seed, counter = self.engine.noise_state()
        return np.array([seed & 0xFFFFFFFF, counter & 0xFFFFFFFF], np.uint32)

    def set_noise_key(self, key) -> None:
        k = np.asarray(key, np.uint64).reshape(-1)
        self.engine.set_noise_state(int(k[0]), int(k[1]))

    def rng_state(self) -> dict:
        return self._rng.bit_generator.state

    def set_rng_state(self, st: dict) -> None:
        self._rng.bit_generator.state = st

    def spawn_replay_buffer(self, env_config, config, seed: int = 1) -> MultiTaskReplayBuffer:
        T = self.num_tasks
        cap, n = config.buffer_size // T, config.batch_size // T
        assert config.batch_size % T == 0
        returns = bool(getattr(config, "returns_normalization", False))
        mode = 2 if returns else int(config.normalize_rewards)  # returns first, as buffers.py:531-538
        if (cap, n, mode) != (self._cfg_kwargs["capacity"], self._cfg_kwargs["batch_per_task"],
                              int(self._cfg_kwargs.get("normalize_rewards", 0))):
            self._rebuild(capacity=cap, batch_per_task=n, normalize_rewards=mode)
        self._buffer = MultiTaskReplayBuffer(config.buffer_size, T, env_config.observation_space,
                                             env_config.action_space, seed=seed,
                                             normalize_rewards=config.normalize_rewards,
                                             returns_normalization=returns, engine=self.engine)
        return self._buffer

    # ------------------------------------------------------------------ algorithm API
    def get_num_params(self) -> dict[str, int]:
        return {"actor_num_params": self.engine.param_count(L.ACTOR),
                "critic_num_params": self.engine.param_count(L.CRITIC)}

    def sample_action(self, observation):
        obs = np.asarray(observation, np.float32)
        eps = self._rng.standard_normal((obs.shape[0], self.engine.action_dim)).astype(np.float32)
        return self, self.engine.sample_action(obs, eps)

    def eval_action(self, observations):
        return self.engine.eval_action(np.asarray(observations, np.float32))

    def update(self, data):
        """mtsac.py:1249-1251: one gradient step on a ReplayBufferSamples batch."""
        n = np.asarray(data.rewards).shape[0] // self.num_tasks
        if n != self._cfg_kwargs["batch_per_task"]:  # raises once a buffer lives in the engine
            self._rebuild(batch_per_task=n, capacity=max(self._cfg_kwargs["capacity"], n))
        self.engine.update(tuple(data))
        return self, _DeviceLogs(self.engine, self.surgery)

    def update_from_buffer(self, replay_buffer, batch_size: int, want_logs: bool):
        if getattr(replay_buffer, "engine", None) is self.engine and batch_size // self.num_tasks == \
                self._cfg_kwargs["batch_per_task"]:
            self.engine.update_many(1)  # device sampling + update, no host round trip
            return self, _DeviceLogs(self.engine, self.surgery)
        return super().update_from_buffer(replay_buffer, batch_size, want_logs)

    # ------------------------------------------------------------------ per-task batch-size sampler
    def setup_task_sampler(self, config) -> None:
        """``sampler_type`` "loss" (Sampler) or "adaptive" (AdaptiveSampler) of mtrl/rl/sampling_algs.py.  The
        reference declares ``sampler_type`` and ``update_weights_every`` and never reads them; this wiring is
        ours: every ``update_weights_every`` gradient steps the last step's per-task critic losses become the
        per-task batch sizes of the following device-sampled steps."""
        kind = getattr(config, "sampler_type", None)
        self._sampler, self._sampler_steps, self._sampler_sizes = None, 0, None
        if kind is None:
            return
        sampler = make_sampler(kind, self.num_tasks)
        if self.surgery:
            raise NotImplementedError(
                f"sampler_type={kind!r} with {_SURGERY[self.surgery][1]}: the gradient-surgery step reads "
                "interleaved rows with the same count for every task (its per-task weight grads stride the batch "
                "by T), so it cannot run on per-task batch sizes")
        if self.engine.T_l != self.num_tasks:
            raise NotImplementedError(
                f"sampler_type={kind!r} on a task-sharded engine: the sizes are normalised over every task's loss "
                "and the batch total is fixed over all tasks, so all tasks must live on one engine")
        self._sampler = sampler
        self._sampler_every = max(1, int(config.update_weights_every))
        self.engine.set_task_loss_logging(True)

    def task_sampler_step(self):
        if self._sampler is None:
            return {}
        self._sampler_steps += 1
        if self._sampler_steps % self._sampler_every:
            return {}
        losses = self.engine.task_losses()[0]  # the critic's
        sizes = np.asarray(self._sampler.sample_batch_sizes(losses, self.engine.B), np.int64)
        self.engine.set_task_batch_sizes(sizes)
        self._sampler_sizes = sizes
        logs = {f"sampler/batch_size_task_{t}": int(sizes[t]) for t in range(self.num_tasks)}
        self.sampler_log_history.append(logs)
        return logs

    def task_sampler_restore(self) -> None:
        if self._sampler_sizes is not None:
            self.engine.set_task_batch_sizes(self._sampler_sizes)

    def compute_weights(self, data):
        """mtsac.py:870-1170: per-task gradient-conflict metrics at evaluation time (no update).
        Per-task gradients, Gram matrix, conflict / support / interference counts on the device
        (mtrl_amd/conflict.py); the 66 log entries of the reference's dict.  The reference
        samples one (n, A) noise draw per vmapped task from a single key (mtsac.py:892, 1052);
        that structure is kept: one draw repeated for every task's rows."""
        from ....conflict import compute_weights

        T, A = self.num_tasks, self.engine.action_dim
        n = np.asarray(data.rewards).shape[0] // T
        if n != self._cfg_kwargs["batch_per_task"]:
            self._rebuild(batch_per_task=n, capacity=max(self._cfg_kwargs["capacity"], n))
        e_next = np.repeat(self._rng.standard_normal((n, A)), T, axis=0).astype(np.float32)  # row i*T + t
        e_cur = np.repeat(self._rng.standard_normal((n, A)), T, axis=0).astype(np.float32)
        return self, compute_weights(self.engine, tuple(data), e_next, e_cur)

    def get_metrics(self, metrics, data):
        """mtsac.py ``get_metrics``: dormant-neuron and srank logs of every trunk layer of the actor and of
        each online critic member at evaluation time (no update), on ``data.observations`` and one action
        sample a ~ pi(.|s).  The statistics and the activation Grams come from one device pass
        (mtrl_amd/netmetrics.py); ``metrics.is_enabled`` decides the groups as the reference's enum does
        (a flag test: NONE nothing, DORMANT_NEURONS / SRANK their own group, ALL both)."""
        from ....netmetrics import compute_metrics
        from ...config.utils import Metrics

        if not (metrics.is_enabled(Metrics.DORMANT_NEURONS) or metrics.is_enabled(Metrics.SRANK)):
            return self, {}
        obs = np.asarray(data.observations, np.float32)
        n = obs.shape[0] // self.num_tasks
        if n != self._cfg_kwargs["batch_per_task"]:  # raises once a buffer lives in the engine
            self._rebuild(batch_per_task=n, capacity=max(self._cfg_kwargs["capacity"], n))
        eps = self._rng.standard_normal((obs.shape[0], self.engine.action_dim)).astype(np.float32)
        # where srank's eigenvalues are solved: "host" (numpy) or "device" 
        eig = os.environ.get("MTSAC_NETWORK_METRICS_EIG", "host")
        return self, compute_metrics(self.engine, metrics, obs, eps, eig=eig)

    # ------------------------------------------------------------------ state (checkpoint)
    def state_dict(self) -> dict[str, np.ndarray]:
        """Agent pytree keyed by flax path (compat/checkpoint.py), e.g.
        ``critic/target_params/VmapQValueFunction_0/MultiHeadNetwork_0/layer_1/kernel``."""
        from ...checkpoint import agent_state

        return agent_state(self)

    def load_state_dict(self, d: Mapping) -> None:
        from ...checkpoint import load_agent_state

        if "tensor_0" in d:  # flat-vector layout of earlier checkpoints
            for w in range(10):
                self.engine.set_params(w, np.asarray(d[f"tensor_{w}"]))
            for i, c in enumerate(np.asarray(d["adam_counts"])):
                self.engine.set_adam_count(i, int(c))
            return
        load_agent_state(self, d)
