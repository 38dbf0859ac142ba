"""Python handle of one HIP MTSAC engine (``libmtsac.so``, include/mtsac.h).

Thin, allocation-free wrapper: it converts arrays to contiguous fp32 host
buffers (numpy) or passes device pointers through (torch CUDA tensors), calls the
C-ABI, and turns negative return codes into :class:`MTSACError`.
"""

from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from . import _lib
from ._lib import LOG_KEYS, Batch, Config, MTSACError, check
# PCGradState fields (mtrl/optim/pcgrad.py:12-17), the order of mtsac_get_pcgrad_logs per network
from .pcgrad import LOG_KEYS as PCGRAD_LOG_KEYS
# CAGradState fields (mtrl/optim/cagrad.py:12-17); mtsac_get_cagrad_logs holds the four scalars, then
# task_weights
from .cagrad import LOG_KEYS as CAGRAD_LOG_KEYS
# GradNormState fields the reference logs (mtrl/optim/gradnorm.py:34-37, mtsac.py:1224-1239): arrays of
# length T; the inner opt_state lives in the checkpoint, not in the logs
from .gradnorm import LOG_KEYS as GRADNORM_LOG_KEYS


def _ptr(x) -> tuple[int, Any]:
    """(address, keep-alive) of a host numpy array or a torch tensor (host or device)."""
    if x is None:
        return 0, None
    if hasattr(x, "data_ptr") and hasattr(x, "is_contiguous"):
        import torch

        t = x
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        return t.data_ptr(), t
    a = np.ascontiguousarray(x, dtype=np.float32)
    return a.ctypes.data, a


def default_config(num_tasks: int) -> Config:
    c = Config()
    _lib.load().mtsac_default_config(ctypes.byref(c), num_tasks)
    return c


def make_config(**kw) -> Config:
    """Config with the C defaults (mtsac_default_config) overridden by ``kw``."""
    c = default_config(int(kw["num_tasks"]))
    for k, v in kw.items():
        if k == "actor_max_grad_norm" or k == "critic_max_grad_norm" or k == "alpha_max_grad_norm":
            v = -1.0 if v is None else v  # None: no clip_by_global_norm in the chain
        setattr(c, k, v)
    return c


class MTSACEngine:
    """One engine per GPU: device-resident replay buffer + MTSAC update."""

    def __init__(self, config: Config, device: int = 0, shared_head: bool = False):
        """shared_head: the reference's VanillaNetwork (MTSAC_NET_SHARED_HEAD): one head layer_D for all tasks,
        parameter vectors in that tree's leaf order (layer_0 .. layer_D, the head last; mtrl_amd.init)."""
        self.lib = _lib.load()
        self.config = config
        self.device = device
        self.shared_head = bool(shared_head)
        h = ctypes.c_void_p()
        flags = _lib.NET_SHARED_HEAD if shared_head else 0
        check(self.lib.mtsac_create_flags(ctypes.byref(config), flags, device, ctypes.byref(h)))
        self._h = h
        c = config
        self.T_l = c.task_count
        self.B = c.batch_per_task * c.task_count
        self.obs_dim = c.obs_dim
        self.action_dim = c.action_dim

    # ------------------------------------------------------------------ lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.mtsac_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def param_count(self, which: int) -> int:
        return check(self.lib.mtsac_param_count(self._h, which))

    def set_params(self, which: int, values) -> None:
        n = self.param_count(which)
        p, keep = _ptr(np.asarray(values, dtype=np.float32).reshape(-1))
        check(self.lib.mtsac_set_params(self._h, which, p, n))

    def get_params(self, which: int) -> np.ndarray:
        n = self.param_count(which)
        out = np.empty(n, dtype=np.float32)
        check(self.lib.mtsac_get_params(self._h, which, out.ctypes.data, n))
        return out

    def set_adam_count(self, which: int, count: int) -> None:
        check(self.lib.mtsac_set_adam_count(self._h, which, count))

    def get_adam_count(self, which: int) -> int:
        c = ctypes.c_int32()
        check(self.lib.mtsac_get_adam_count(self._h, which, ctypes.byref(c)))
        return c.value

    def opt_form(self, which: int) -> int:
        """Form of the fused optimizer pass of the actor (0) or critic (1): bits 0-1 0 elementwise,
        1 plane segments, 2 tiles; bit 4 transposed head kernel written; bit 5 sharded
        (include/mtsac_debug.h mtsac_debug_opt_form)."""
        return check(self.lib.mtsac_debug_opt_form(self._h, which))

    # ------------------------------------------------------------------ replay buffer
    def buffer_add(self, obs, next_obs, actions, rewards, dones) -> None:
        """Non-blocking add.  Device (torch) tensors are read in the order of torch's current
        stream, which then waits for the read (mtsac_buffer_add_stream): they may be reused or
        freed as soon as this returns."""
        args = [_ptr(x) for x in (obs, next_obs, actions, rewards, dones)]
        stream = None
        if getattr(obs, "is_cuda", False):
            import torch

            stream = torch.cuda.current_stream(obs.device).cuda_stream
        check(self.lib.mtsac_buffer_add_stream(self._h, *[a[0] for a in args], stream))

    def buffer_write(self, slot_begin: int, obs, next_obs, actions, rewards, dones) -> None:
        n = int(np.asarray(rewards).size) // self.T_l  # slots (rows are slot-major, T_l per slot)
        args = [_ptr(x) for x in (obs, next_obs, actions, rewards, dones)]
        check(self.lib.mtsac_buffer_write(self._h, slot_begin, n, *[a[0] for a in args]))

    def buffer_read(self, slot_begin: int, n_slots: int):
        T, D, A = self.T_l, self.obs_dim, self.action_dim
        obs = np.empty((n_slots, T, D), np.float32)
        nobs = np.empty((n_slots, T, D), np.float32)
        act = np.empty((n_slots, T, A), np.float32)
        rew = np.empty((n_slots, T), np.float32)
        done = np.empty((n_slots, T), np.float32)
        check(self.lib.mtsac_buffer_read(self._h, slot_begin, n_slots, obs.ctypes.data, nobs.ctypes.data,
                                         act.ctypes.data, rew.ctypes.data, done.ctypes.data))
        return obs, nobs, act, rew, done

    def buffer_fill_synthetic(self, seed: int = 1234) -> None:
        check(self.lib.mtsac_buffer_fill_synthetic(self._h, seed))

    def buffer_state(self) -> tuple[int, bool]:
        pos, full = ctypes.c_int64(), ctypes.c_int32()
        check(self.lib.mtsac_buffer_get_state(self._h, ctypes.byref(pos), ctypes.byref(full)))
        return pos.value, bool(full.value)

    def set_buffer_state(self, pos: int, full: bool) -> None:
        check(self.lib.mtsac_buffer_set_state(self._h, pos, 1 if full else 0))

    def set_reward_stats(self, min_r, max_r) -> None:
        mn = np.ascontiguousarray(min_r, dtype=np.float64)
        mx = np.ascontiguousarray(max_r, dtype=np.float64)
        check(self.lib.mtsac_buffer_set_reward_stats(self._h, mn.ctypes.data_as(_lib.PD), mx.ctypes.data_as(_lib.PD)))

    def reward_stats(self) -> tuple[np.ndarray, np.ndarray]:
        mn, mx = np.empty(self.T_l, np.float64), np.empty(self.T_l, np.float64)
        check(self.lib.mtsac_buffer_get_reward_stats(self._h, mn.ctypes.data_as(_lib.PD), mx.ctypes.data_as(_lib.PD)))
        return mn, mx

    def set_rng_state(self, st: dict) -> None:
        """Load a numpy ``PCG64`` ``bit_generator.state`` dict (buffers.py:335)."""
        assert st["bit_generator"] == "PCG64"
        s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
        m = (1 << 64) - 1
        check(self.lib.mtsac_rng_set(self._h, s >> 64, s & m, inc >> 64, inc & m, int(st["has_uint32"]),
                                     int(st["uinteger"])))

    def get_rng_state(self) -> dict:
        v = [ctypes.c_uint64() for _ in range(4)]
        has, u = ctypes.c_int32(), ctypes.c_uint32()
        check(self.lib.mtsac_rng_get(self._h, *[ctypes.byref(x) for x in v], ctypes.byref(has), ctypes.byref(u)))
        return {
            "bit_generator": "PCG64",
            "state": {"state": (v[0].value << 64) | v[1].value, "inc": (v[2].value << 64) | v[3].value},
            "has_uint32": has.value,
            "uinteger": u.value,
        }

    def seed_rng(self, seed) -> None:
        """Seed the index stream exactly like ``np.random.default_rng(seed)`` (buffers.py:260)."""
        self.set_rng_state(np.random.default_rng(seed).bit_generator.state)

    def sample(self):
        """(indices, (obs, act, next_obs, done, rew)) of one device sample: ``batch_per_task`` indices and
        interleaved rows i*T + t, or, with per-task batch sizes set, one index per row and task-major rows."""
        n = self.config.batch_per_task
        B, D, A = self.B, self.obs_dim, self.action_dim
        idx = np.empty(B if self.task_batch_sizes_set() else n, np.int64)
        obs, nobs = np.empty((B, D), np.float32), np.empty((B, D), np.float32)
        act, done, rew = np.empty((B, A), np.float32), np.empty((B, 1), np.float32), np.empty((B, 1), np.float32)
        check(self.lib.mtsac_sample(self._h, idx.ctypes.data, obs.ctypes.data, act.ctypes.data, nobs.ctypes.data,
                                    done.ctypes.data, rew.ctypes.data))
        return idx, (obs, act, nobs, done, rew)

    # ------------------------------------------------------------------ per-task batch sizes (include/mtsac.h)
    def set_task_batch_sizes(self, sizes) -> None:
        """Per-task batch sizes [T] (>= 0, summing to B) for the step's own device sampling -- ``sample``,
        ``update()`` without a batch, ``update_many`` -- or None: back to ``batch_per_task`` rows per task."""
        if sizes is None:
            check(self.lib.mtsac_set_task_batch_sizes(self._h, None))
            return
        a = np.asarray(sizes)
        if a.shape != (self.T_l,):
            raise ValueError(f"task batch sizes must have shape ({self.T_l},), got {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("task batch sizes must be integers")
        a = np.ascontiguousarray(a, np.int32)
        check(self.lib.mtsac_set_task_batch_sizes(self._h, a.ctypes.data))

    def task_batch_sizes_set(self) -> bool:
        out = np.empty(self.T_l, np.int32)
        return check(self.lib.mtsac_get_task_batch_sizes(self._h, out.ctypes.data)) == 1

    def task_batch_sizes(self) -> np.ndarray:
        """The sizes in force (``batch_per_task`` each when none are set)."""
        out = np.empty(self.T_l, np.int32)
        check(self.lib.mtsac_get_task_batch_sizes(self._h, out.ctypes.data))
        return out

    def set_task_loss_logging(self, on: bool) -> None:
        """Per-task loss terms of the plain step (one more launch per step while on)."""
        check(self.lib.mtsac_set_task_loss_logging(self._h, 1 if on else 0))

    def task_losses(self) -> np.ndarray:
        """[2][T]: the last plain step's per-task mean critic (0) and actor (1) loss terms; 0 for a task
        without rows."""
        out = np.empty((2, self.T_l), np.float32)
        check(self.lib.mtsac_get_task_losses(self._h, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ update
    def update(self, batch=None, eps_next=None, eps_cur=None) -> None:
        keep = []
        bp = None
        if batch is not None:
            obs, act, nobs, done, rew = batch
            ptrs = [_ptr(x) for x in (obs, act, nobs, done, rew)]
            keep.extend(ptrs)
            b = Batch(*[p[0] for p in ptrs])
            bp = ctypes.byref(b)
        en, ec = _ptr(eps_next), _ptr(eps_cur)
        keep.extend([en, ec])
        check(self.lib.mtsac_update(self._h, bp, en[0] or None, ec[0] or None))

    # ------------------------------------------------------------------ gradient-conflict metrics
    def task_gradients(self, batch=None, eps_next=None, eps_cur=None) -> None:
        """Per-task gradients on the current parameters (include/mtsac.h, mtsac_task_gradients)."""
        keep = []
        bp = None
        if batch is not None:
            ptrs = [_ptr(x) for x in batch]
            keep.extend(ptrs)
            b = Batch(*[p[0] for p in ptrs])
            bp = ctypes.byref(b)
        en, ec = _ptr(eps_next), _ptr(eps_cur)
        keep.extend([en, ec])
        check(self.lib.mtsac_task_gradients(self._h, bp, en[0] or None, ec[0] or None))

    def task_gradient_size(self, which: int) -> int:
        return check(self.lib.mtsac_task_gradient_size(self._h, which))

    def get_task_gradients(self, which: int) -> np.ndarray:
        P = self.task_gradient_size(which)
        out = np.empty((self.T_l, P), np.float32)
        check(self.lib.mtsac_get_task_gradients(self._h, which, out.ctypes.data, out.size))
        return out

    def set_task_gradients(self, which: int, G) -> None:
        G = np.ascontiguousarray(G, np.float32)
        check(self.lib.mtsac_set_task_gradients(self._h, which, G.ctypes.data, G.size))

    def task_gradient_select(self, which: int, ranks) -> np.ndarray:
        r = np.ascontiguousarray(ranks, np.int64).reshape(self.T_l, 2)
        out = np.empty((self.T_l, 2), np.float32)
        check(self.lib.mtsac_task_gradient_select(self._h, which, r.ctypes.data, out.ctypes.data))
        return out

    def task_gradient_stats(self, which: int, thresholds, eps: float, tau: float) -> dict:
        T = self.T_l
        thr = np.ascontiguousarray(thresholds, np.float32).reshape(T)
        gram, l1 = np.empty((T, T), np.float64), np.empty(T, np.float64)
        counts, nz = np.empty((4, T, T), np.int64), np.empty(T, np.int64)
        check(self.lib.mtsac_task_gradient_stats(self._h, which, thr.ctypes.data, eps, tau, gram.ctypes.data,
                                                 l1.ctypes.data, counts.ctypes.data, nz.ctypes.data))
        return {"gram": gram, "l1": l1, "conflict": counts[0], "intersection": counts[1], "genuine": counts[2],
                "mismatch": counts[3], "near_zero": nz}

    # ------------------------------------------------------------------ network health metrics
    def network_metrics(self, observations=None, eps=None, dormant: bool = True, gram: bool = True,
                        threshold: float = 0.1, eig: str = "host") -> dict:
        """Dormant-neuron statistics and activation Grams of every trunk layer (include/mtsac.h,
        mtsac_network_metrics), nothing updated.  ``observations`` [B][obs_dim] (rows interleaved i*T + t) or
        None (a device sample); ``eps`` [B][A] or None (device noise).  Returns ``{"actor": r, "critic": r}`` with
        ``r = {"members": E, "depth": D, "width": W, "scores": [E][D][W] float32 normalised scores,
        "counts": [E][D] int32, "gram": E lists of D float64 [r][r] matrices}`` (the parts not asked for: None).
        ``eig="device"`` with ``gram``: the Grams stay on the device and are solved there (``network_eigvals``);
        ``r["gram"]`` is None and ``r["eigvals"]`` [E][D][r] float64 ascending, ``r["eig_flags"]`` [E][D] int32.
        mtrl_amd/netmetrics.py makes the LogDict of them."""
        if eig not in ("host", "device"):
            raise ValueError(f"eig must be 'host' or 'device', not {eig!r}")
        c = self.config
        what = (1 if dormant else 0) | (2 if gram else 0)
        bp, keep = None, None
        if observations is not None:
            keep = _ptr(observations)
            b = Batch(keep[0], None, None, None, None)
            bp = ctypes.byref(b)
        ep = _ptr(eps)
        check(self.lib.mtsac_network_metrics(self._h, bp, ep[0] or None, what, float(threshold)))
        out = {}
        for which, (name, W, D, E) in enumerate((("actor", c.actor_width, c.actor_depth, 1),
                                                 ("critic", c.critic_width, c.critic_depth, c.num_critics))):
            r = {"members": E, "depth": D, "width": W, "scores": None, "counts": None, "gram": None}
            if dormant:
                r["scores"], r["counts"] = np.empty((E, D, W), np.float32), np.empty((E, D), np.int32)
                check(self.lib.mtsac_get_network_scores(self._h, which, r["scores"].ctypes.data,
                                                        r["counts"].ctypes.data))
            if gram and eig == "device":
                r["eigvals"], r["eig_flags"] = self.network_eigvals(which)
            elif gram:
                n = check(self.lib.mtsac_network_gram_dim(self._h, which))
                r["gram"] = [[np.empty((n, n), np.float64) for _ in range(D)] for _ in range(E)]
                for e in range(E):
                    for i in range(D):
                        check(self.lib.mtsac_get_network_gram(self._h, which, e, i, r["gram"][e][i].ctypes.data))
            out[name] = r
        return out

    def network_eigvals(self, which: int):
        """Eigenvalues of the Grams of the last ``network_metrics`` call with ``gram``, solved on the device
        (mtsac_network_eigvals).  ``which``: 0 actor, 1 critic.  Returns
        ``(lam [E][D][r] float64 ascending, flags [E][D] int32)``; a nonzero flag marks a Gram with a non-finite
        entry, whose eigenvalues are NaN.  The solve consumes the Grams of ``which``."""
        c = self.config
        E, D = ((1, c.actor_depth), (c.num_critics, c.critic_depth))[which]
        n = check(self.lib.mtsac_network_gram_dim(self._h, which))
        lam, flags = np.empty((E, D, n), np.float64), np.empty((E, D), np.int32)
        check(self.lib.mtsac_network_eigvals(self._h, which, lam.ctypes.data, flags.ctypes.data))
        return lam, flags

    def network_eigvals_kernel_ms(self, which: int) -> tuple[float, float, int]:
        """HIP-event time (ms) of the last ``network_eigvals(which)``: reduction, bisection; and its launches."""
        ms, n = (ctypes.c_double * 2)(), ctypes.c_int32(0)
        check(self.lib.mtsac_debug_network_eigvals_ms(self._h, which, ms, ctypes.byref(n)))
        return float(ms[0]), float(ms[1]), int(n.value)

    def network_metrics_kernel_ms(self) -> tuple[float, float]:
        """HIP-event time of the last network_metrics call's statistics and Gram kernels (ms)."""
        ms = (ctypes.c_double * 2)()
        check(self.lib.mtsac_debug_network_metrics_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    # ------------------------------------------------------------------ PCGrad (include/mtsac.h)
    def set_pcgrad(self, on: bool, cosine_sim_logs: bool = False) -> None:
        """PCGrad on both optimizers: update / update_many run the gradient-surgery step."""
        check(self.lib.mtsac_set_pcgrad(self._h, 1 if on else 0, 1 if cosine_sim_logs else 0))

    def pcgrad_set_order(self, critic_perm=None, actor_perm=None) -> None:
        """Pin the task orders of the following steps; None, None: device draws."""
        if critic_perm is None and actor_perm is None:
            check(self.lib.mtsac_pcgrad_set_order(self._h, None, None))
            return
        c = np.ascontiguousarray(critic_perm, np.int32).reshape(self.T_l)
        a = np.ascontiguousarray(actor_perm, np.int32).reshape(self.T_l)
        check(self.lib.mtsac_pcgrad_set_order(self._h, c.ctypes.data, a.ctypes.data))

    def pcgrad_get_order(self) -> tuple[np.ndarray, np.ndarray]:
        c, a = np.empty(self.T_l, np.int32), np.empty(self.T_l, np.int32)
        check(self.lib.mtsac_pcgrad_get_order(self._h, c.ctypes.data, a.ctypes.data))
        return c, a

    def pcgrad_logs(self) -> dict[str, float]:
        out = np.empty(2 * len(PCGRAD_LOG_KEYS), np.float32)
        check(self.lib.mtsac_get_pcgrad_logs(self._h, out.ctypes.data))
        return {f"metrics/{net}_{k}": float(out[5 * w + i])
                for w, net in enumerate(("critic", "actor")) for i, k in enumerate(PCGRAD_LOG_KEYS)}

    def task_gram(self, which: int) -> np.ndarray:
        g = np.empty((self.T_l, self.T_l), np.float64)
        check(self.lib.mtsac_task_gram(self._h, which, g.ctypes.data))
        return g

    def task_pcgrad_solve(self, which: int, perm, cosine_sim_logs: bool = False):
        """(w [T] float32, logs: the five PCGradState values and ``grad_magnitude``) of the device solve."""
        p = np.ascontiguousarray(perm, np.int32).reshape(self.T_l)
        w, logs = np.empty(self.T_l, np.float32), np.empty(6, np.float32)
        check(self.lib.mtsac_task_pcgrad_solve(self._h, which, p.ctypes.data, 1 if cosine_sim_logs else 0,
                                               w.ctypes.data, logs.ctypes.data))
        return w, {k: float(v) for k, v in zip(PCGRAD_LOG_KEYS + ("grad_magnitude",), logs)}

    def task_combine(self, which: int, w) -> np.ndarray:
        w = np.ascontiguousarray(w, np.float32).reshape(self.T_l)
        out = np.empty(self.task_gradient_size(which), np.float32)
        check(self.lib.mtsac_task_combine(self._h, which, w.ctypes.data, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ CAGrad (include/mtsac.h)
    def set_cagrad(self, on: bool, c: float = 0.5, num_iterations: int = 21, learning_rate: float | None = None,
                   momentum: float = 0.5, cosine_sim_logs: bool = False) -> None:
        """CAGrad on both optimizers: update / update_many run the CAGrad step.  The defaults are the
        reference's (learning_rate None: 25 below 50 tasks, 50 from there on)."""
        lr = (25.0 if self.T_l < 50 else 50.0) if learning_rate is None else float(learning_rate)
        check(self.lib.mtsac_set_cagrad(self._h, 1 if on else 0, float(c), int(num_iterations), lr, float(momentum),
                                        1 if cosine_sim_logs else 0))

    def cagrad_logs(self) -> dict:
        """``metrics/{critic,actor}_<CAGradState field>``; task_weights a float32 array of length T."""
        T = self.T_l
        out = np.empty(2 * (4 + T), np.float32)
        check(self.lib.mtsac_get_cagrad_logs(self._h, out.ctypes.data))
        logs = {}
        for w, net in enumerate(("critic", "actor")):
            o = (4 + T) * w
            logs[f"metrics/{net}_task_weights"] = out[o + 4:o + 4 + T].copy()
            for i, k in enumerate(CAGRAD_LOG_KEYS[1:]):
                logs[f"metrics/{net}_{k}"] = float(out[o + i])
        return logs

    def task_cagrad_solve(self, which: int, c: float = 0.5, num_iterations: int = 21,
                          learning_rate: float | None = None, momentum: float = 0.5, w0=None,
                          cosine_sim_logs: bool = False):
        """(w [T] float32 combine weights on the raw rows, logs) of the device solve on the matrix
        set_task_gradients / task_gradients left: logs holds the CAGradState fields, ``grad_magnitude``,
        ``best_iteration`` and ``obj_hist`` [num_iterations] (float64).  ``w0``: the search's start
        (None: zeros, the reference's)."""
        T = self.T_l
        lr = (25.0 if T < 50 else 50.0) if learning_rate is None else float(learning_rate)
        w0a = None if w0 is None else np.ascontiguousarray(w0, np.float64).reshape(T)
        n = max(int(num_iterations), 1)
        w, tw, lg, hist = np.empty(T, np.float32), np.empty(T, np.float32), np.empty(6, np.float32), np.empty(n)
        check(self.lib.mtsac_task_cagrad_solve(self._h, which, float(c), int(num_iterations), lr, float(momentum),
                                               None if w0a is None else w0a.ctypes.data,
                                               1 if cosine_sim_logs else 0, w.ctypes.data, tw.ctypes.data,
                                               lg.ctypes.data, hist.ctypes.data))
        logs = {"task_weights": tw}
        logs.update({k: float(v) for k, v in zip(CAGRAD_LOG_KEYS[1:], lg[:4])})
        logs.update(best_iteration=int(lg[4]), grad_magnitude=float(lg[5]), obj_hist=hist)
        return w, logs

    # ------------------------------------------------------------------ GradNorm (include/mtsac.h)
    @staticmethod
    def _pair(v, dtype, none=None):
        """A per-network value (critic, actor) from a scalar or a pair; None -> ``none``."""
        v = tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else (v, v)
        return np.array([none if x is None else x for x in v], dtype).reshape(2)

    def set_gradnorm(self, on: bool, asymmetry: float = 0.12, per_task_clip=True, inner_lr=3e-4, inner_eps=1e-5,
                     inner_max_grad_norm=1.0, initial_weights=None, weighted_norms: bool = False) -> None:
        """GradNorm on both optimizers: update / update_many run the GradNorm step, from a freshly
        initialised state.  ``per_task_clip`` (bool(GradNormConfig.max_grad_norm)), ``inner_lr``,
        ``inner_eps`` and ``inner_max_grad_norm`` (None: no clip) are scalars or (critic, actor) pairs;
        ``initial_weights``: None (ones), [T] for both networks or [2][T].  ``weighted_norms``: the form the
        reference has commented out (mtrl_amd/gradnorm.py)."""
        T = self.T_l
        clip = self._pair(per_task_clip, np.int32)
        lr, eps = self._pair(inner_lr, np.float64), self._pair(inner_eps, np.float64)
        mx = self._pair(inner_max_grad_norm, np.float64, none=-1.0)
        iw = None
        if initial_weights is not None:
            iw = np.ascontiguousarray(np.broadcast_to(np.asarray(initial_weights, np.float32), (2, T)))
        check(self.lib.mtsac_set_gradnorm(self._h, 1 if on else 0, float(asymmetry), clip.ctypes.data, lr.ctypes.data,
                                          eps.ctypes.data, mx.ctypes.data, None if iw is None else iw.ctypes.data,
                                          1 if weighted_norms else 0))

    def gradnorm_state(self, which: int):
        """The ``mtrl_amd.gradnorm.GradNormState`` of one network (0 critic, 1 actor)."""
        from .gradnorm import GradNormState

        T = self.T_l
        a = [np.empty(T, np.float32) for _ in range(4)]
        n = ctypes.c_int64(0)
        check(self.lib.mtsac_gradnorm_get_state(self._h, which, *(x.ctypes.data for x in a), ctypes.addressof(n)))
        return GradNormState(task_weights=a[0], original_losses=a[1], count=int(n.value), mu=a[2], nu=a[3])

    def set_gradnorm_state(self, which: int, state) -> None:
        a = [np.ascontiguousarray(x, np.float32).reshape(self.T_l)
             for x in (state.task_weights, state.original_losses, state.mu, state.nu)]
        check(self.lib.mtsac_gradnorm_set_state(self._h, which, *(x.ctypes.data for x in a), int(state.count)))

    def gradnorm_logs(self) -> dict:
        """``metrics/{critic,actor}_{task_weights,original_losses}`` (float32 arrays of length T) and
        ``metrics/{critic,actor}_gradnorm_loss``."""
        T = self.T_l
        out = np.empty(2 * (2 * T + 1), np.float32)
        check(self.lib.mtsac_get_gradnorm_logs(self._h, out.ctypes.data))
        logs = {}
        for w, net in enumerate(("critic", "actor")):
            o = (2 * T + 1) * w
            logs[f"metrics/{net}_task_weights"] = out[o:o + T].copy()
            logs[f"metrics/{net}_original_losses"] = out[o + T:o + 2 * T].copy()
            logs[f"metrics/{net}_gradnorm_loss"] = float(out[o + 2 * T])
        return logs

    def gradnorm_task_losses(self) -> np.ndarray:
        """[2][T]: the per-task loss values the last GradNorm step's solves read (critic, actor)."""
        out = np.empty((2, self.T_l), np.float32)
        check(self.lib.mtsac_get_gradnorm_task_losses(self._h, out.ctypes.data))
        return out

    def task_gradnorm_solve(self, which: int, task_losses, state, asymmetry: float = 0.12, per_task_clip: bool = True,
                            inner_lr: float = 3e-4, inner_eps: float = 1e-5, inner_max_grad_norm: float | None = 1.0,
                            weighted_norms: bool = False):
        """(w [T] float32 combine weights on the raw rows, new GradNormState, logs) of the device solve on
        the matrix set_task_gradients / task_gradients left; the arguments of
        ``mtrl_amd.gradnorm.gradnorm_from_gram``.  logs: task_weights, original_losses, gradnorm_loss,
        sign_margin, grad_magnitude."""
        from .gradnorm import GradNormState

        T = self.T_l
        ls = np.ascontiguousarray(task_losses, np.float32).reshape(T)
        a = [np.array(x, np.float32).reshape(T) for x in (state.task_weights, state.original_losses, state.mu, state.nu)]
        n = ctypes.c_int64(int(state.count))
        w, lg = np.empty(T, np.float32), np.empty(3, np.float32)
        check(self.lib.mtsac_task_gradnorm_solve(
            self._h, which, ls.ctypes.data, float(asymmetry), 1 if per_task_clip else 0, float(inner_lr),
            float(inner_eps), -1.0 if inner_max_grad_norm is None else float(inner_max_grad_norm),
            1 if weighted_norms else 0, *(x.ctypes.data for x in a), ctypes.addressof(n), w.ctypes.data,
            lg.ctypes.data))
        new = GradNormState(task_weights=a[0], original_losses=a[1], count=int(n.value), mu=a[2], nu=a[3])
        logs = {"task_weights": a[0], "original_losses": a[1], "gradnorm_loss": float(lg[0]),
                "sign_margin": float(lg[1]), "grad_magnitude": float(lg[2])}
        return w, new, logs

    def update_many(self, steps: int) -> None:
        check(self.lib.mtsac_update_many(self._h, steps))

    def logs(self) -> dict[str, float]:
        out = np.empty(_lib.NUM_LOGS, np.float32)
        check(self.lib.mtsac_get_logs(self._h, out.ctypes.data))
        return {k: float(v) for k, v in zip(LOG_KEYS, out)}

    def enable_graph(self, on: bool) -> None:
        check(self.lib.mtsac_enable_graph(self._h, 1 if on else 0))

    def synchronize(self) -> None:
        check(self.lib.mtsac_synchronize(self._h))

    # ------------------------------------------------------------------ rollout
    def eval_action(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out = np.empty((obs.shape[0], self.action_dim), np.float32)
        check(self.lib.mtsac_eval_action(self._h, obs.ctypes.data, obs.shape[0], out.ctypes.data))
        return out

    def sample_action(self, obs, eps) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        eps = np.ascontiguousarray(eps, dtype=np.float32)
        out = np.empty((obs.shape[0], self.action_dim), np.float32)
        check(self.lib.mtsac_sample_action(self._h, obs.ctypes.data, obs.shape[0], eps.ctypes.data, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _lib.load()
        n = lib.mtsac_comm_unique_id_size()
        buf = ctypes.create_string_buffer(n)
        check(lib.mtsac_comm_get_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, nranks: int, rank: int, timeout_s: float = 0.0) -> None:
        """Join the RCCL communicator; timeout_s > 0 raises MTSACError (-110) when the peers have
        not all joined by then (include/mtsac.h, mtsac_comm_init_timeout)."""
        buf = ctypes.create_string_buffer(bytes(unique_id), len(unique_id))
        check(self.lib.mtsac_comm_init_timeout(self._h, buf, nranks, rank, float(timeout_s)))

    def noise_state(self) -> tuple[int, int]:
        s, c = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.mtsac_get_noise_state(self._h, ctypes.byref(s), ctypes.byref(c)))
        return s.value, c.value

    def set_noise_state(self, seed: int, counter: int) -> None:
        check(self.lib.mtsac_set_noise_state(self._h, seed, counter))

    def comm_nranks(self) -> int:
        n = ctypes.c_int32()
        check(self.lib.mtsac_comm_nranks(self._h, ctypes.byref(n)))
        return n.value

    def set_allreduce_hook(self, fn) -> None:
        """``fn(device_ptr: int, count: int)`` must leave the SUM over shards in the buffer."""
        if fn is None:
            self._hook = None
            check(self.lib.mtsac_set_allreduce_hook(self._h, None, None))
            return

        def tramp(_user, ptr, count):
            try:
                fn(ptr, count)
                return 0
            except Exception:  # pragma: no cover - reported through the engine
                import traceback

                traceback.print_exc()
                return -1

        self._hook = _lib.ALLREDUCE_FN(tramp)
        check(self.lib.mtsac_set_allreduce_hook(self._h, ctypes.cast(self._hook, ctypes.c_void_p), None))

    def set_collective_hook(self, fn, rank: int, world: int) -> None:
        """``fn(op, device_ptr, count)``: op 0 all-reduce (sum), 1 reduce-scatter in place (this rank's
        shard [rank count / world, (rank + 1) count / world) must hold the sum), 2 all-gather in place
        (include/mtsac.h mtsac_set_collective_hook)."""
        if fn is None:
            self._hook = None
            check(self.lib.mtsac_set_collective_hook(self._h, None, None, 0, 1))
            return

        def tramp(_user, op, ptr, count):
            try:
                fn(op, ptr, count)
                return 0
            except Exception:  # pragma: no cover - reported through the engine
                import traceback

                traceback.print_exc()
                return -1

        self._hook = _lib.COLLECTIVE_FN(tramp)
        check(self.lib.mtsac_set_collective_hook(self._h, ctypes.cast(self._hook, ctypes.c_void_p), None, rank, world))

    def set_sharded_optimizer(self, on: bool) -> None:
        """ZeRO-1-style sharded trunk optimizer for task-sharded runs (include/mtsac.h
        mtsac_set_sharded_optimizer): reduce-scatter, Adam on 1/world of the trunk, all-gather."""
        check(self.lib.mtsac_set_sharded_optimizer(self._h, 1 if on else 0))

    # ------------------------------------------------------------------ measurement
    def set_timing(self, on: bool, serial: bool = False) -> None:
        """HIP-event timing of every GEMM launch of the next update call(s); serial=True runs
        the step on one stream (solo kernel durations), else the step keeps its streams."""
        check(self.lib.mtsac_set_timing(self._h, (2 if serial else 1) if on else 0))

    def timing_kernel(self, family: int) -> str:
        buf = ctypes.create_string_buffer(256)
        check(self.lib.mtsac_get_timing_kernel(self._h, family, buf, 256))
        return buf.value.decode()

    def timing(self, family: int) -> tuple[float, int, float]:
        ms, n, fl = ctypes.c_double(), ctypes.c_int32(), ctypes.c_double()
        check(self.lib.mtsac_get_timing(self._h, family, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        return ms.value, n.value, fl.value


def debug_gemm(kind: int, epi: int, A, B, C, M: int, N: int, K: int, batch: int = 1, a_shared: bool = False,
               bias=None, mask=None, want_db: bool = False, precision: int = 0, splits: int = 1):
    """Run one device GEMM (include/mtsac_debug.h) on host arrays; returns (C, db)."""
    lib = _lib.load()
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    C = np.ascontiguousarray(C, np.float32).copy()
    lda, ldb, ldc = A.shape[-1], B.shape[-1], C.shape[-1]
    bias_a = None if bias is None else np.ascontiguousarray(bias, np.float32)
    mask_a = None if mask is None else np.ascontiguousarray(mask, np.float32)
    db = np.zeros((batch, N), np.float32) if want_db else None
    check(lib.mtsac_debug_gemm(precision | (splits << 8), kind, epi, batch, M, N, K, A.ctypes.data, lda, 1 if a_shared else 0, B.ctypes.data,
                               ldb, C.ctypes.data, ldc, None if bias_a is None else bias_a.ctypes.data,
                               None if mask_a is None else mask_a.ctypes.data,
                               0 if mask_a is None else mask_a.shape[-1], None if db is None else db.ctypes.data))
    return C, db
