"""Shapes, size vectors and numpy references shared by the per-task batch-size tests
(test_task_batch_cpu.py on the CPU, test_gpu_task_batch_*.py on the GPU).

``reference_sample`` states the array branch of the reference's ``MultiTaskReplayBuffer.sample``
(mtrl/rl/buffers.py:496-519) in numpy on a host copy of the store: for every task with a positive size, in task
order, one ``rng.integers(0, max(buffer_size, size), size=size)`` call and the rows ``store[idx, task]``,
concatenated task by task, rewards as stored.  The reference asserts ``sum == 128 * T``; here the total is the
engine's batch ``n * T``.
"""

from __future__ import annotations

import numpy as np

# (T, n, W, A, E): the small shapes of tests/test_gpu_shared_head_update.py
SHAPES = {"t1": (1, 5, 36, 4, 2), "t3": (3, 8, 36, 1, 1), "t4": (4, 5, 260, 6, 3)}
SIZES = {
    "t1": [(5,)],
    "t3": [(24, 0, 0), (1, 0, 23), (9, 8, 7), (8, 8, 8)],
    "t4": [(0, 20, 0, 0), (7, 6, 4, 3)],
}
CASES = [(name, sizes) for name in SHAPES for sizes in SIZES[name]]
CASE_IDS = [f"{name}-{'_'.join(map(str, sizes))}" for name, sizes in CASES]
CAPACITY = 64  # slots per task of every test engine: no size above it


def make_store(T: int, A: int, capacity: int, seed: int, pin_max: bool = False):
    """obs, next_obs [cap][T][39 + T], actions [cap][T][A], rewards, dones [cap][T]: float32, every value its own.
    pin_max: features clipped to +-3.5 and feature 0 of every observation set to 3.75, so that the largest input
    magnitude of ANY set of rows is 3.75 -- split2h takes its input planes' exponent from the stored rows' maximum
    for a device sample and from the batch's own for a user batch, and the two then agree."""
    rng = np.random.default_rng(seed)
    D = 39 + T
    obs, nobs = np.zeros((capacity, T, D), np.float32), np.zeros((capacity, T, D), np.float32)
    obs[..., :39] = rng.standard_normal((capacity, T, 39))
    nobs[..., :39] = rng.standard_normal((capacity, T, 39))
    if pin_max:
        obs[..., :39], nobs[..., :39] = np.clip(obs[..., :39], -3.5, 3.5), np.clip(nobs[..., :39], -3.5, 3.5)
        obs[..., 0] = 3.75
    for t in range(T):
        obs[:, t, 39 + t] = nobs[:, t, 39 + t] = 1.0
    act = rng.uniform(-1, 1, (capacity, T, A)).astype(np.float32)
    rew = rng.uniform(0, 10, (capacity, T)).astype(np.float32)
    done = (rng.uniform(size=(capacity, T)) < 0.2).astype(np.float32)
    return obs, nobs, act, rew, done


def task_indices(rng: np.random.Generator, sizes, buffer_size: int) -> list[np.ndarray]:
    """One ``integers`` call per non-empty task, in task order (an empty task: no call, an empty array)."""
    out = []
    for s in sizes:
        s = int(s)
        out.append(rng.integers(low=0, high=max(buffer_size, s), size=(s,)) if s > 0 else np.zeros(0, np.int64))
    return out


def reference_sample(store, rng: np.random.Generator, sizes, buffer_size: int, total: int):
    """(indices per task, (obs, act, next_obs, done [B][1], rew [B][1], task [B])) of buffers.py:496-519."""
    obs, nobs, act, rew, done = store
    T = obs.shape[1]
    sizes = np.asarray(sizes)
    assert len(sizes) == T
    assert sizes.sum() == total
    idx = task_indices(rng, sizes, buffer_size)
    parts = [[], [], [], [], [], []]
    for t in range(T):
        if sizes[t] > 0:
            i = idx[t]
            for p, x in zip(parts, (obs[i, t], act[i, t], nobs[i, t], done[i, t, None], rew[i, t, None],
                                    np.full(len(i), t, np.int32))):
                p.append(x)
    return idx, tuple(np.concatenate(p, axis=0) for p in parts)


def fill_engine(eng, store, slots: int | None = None) -> None:
    """The whole store into the engine's device buffer, which then counts ``slots`` of them as filled (None: all,
    a full buffer).  Slots past ``slots`` keep valid rows: a size above the fill level samples them (the reference
    reads whatever its arrays hold there), and the engine checks every gathered row's one-hot."""
    obs, nobs, act, rew, done = store
    cap, T = rew.shape
    eng.buffer_write(0, obs.reshape(cap * T, -1), nobs.reshape(cap * T, -1), act.reshape(cap * T, -1),
                     rew.reshape(-1), done.reshape(-1))
    eng.set_buffer_state(0 if slots is None else slots, slots is None)
