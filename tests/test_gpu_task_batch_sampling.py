"""Per-task batch sizes on the device, the sampling half: the index stream (replay_indices_tasks) bit for bit
against numpy's Generator(PCG64) -- one ``integers`` call per non-empty task on one continuous stream -- and the
task-major gather against a numpy gather from the same store, alone (the guarded debug entries) and through the
engine (mtsac_set_task_batch_sizes + mtsac_sample).  Nothing here has a tolerance: every value is compared exactly
(the planes on their raw words, after tests/test_gpu_replay_kernels.py)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import replay_ref as RR
import task_batch_cases as tc

pytestmark = pytest.mark.gpu

PV = ctypes.c_void_p
PAD = 70
M64 = (1 << 64) - 1


def _words(rng: np.random.Generator) -> list[int]:
    st = rng.bit_generator.state
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    return [s >> 64, s & M64, inc >> 64, inc & M64, int(st["has_uint32"]), int(st["uinteger"])]


def _kernel_indices(words, size, sizes):
    from mtrl_amd import _lib as L

    st = np.array(words, np.uint64)
    sz = np.ascontiguousarray(sizes, np.int32)
    total = int(sz.sum())
    idx = np.zeros(total + PAD, np.int32)
    L.check(L.load().mtsac_debug_replay_indices_tasks(st.ctypes.data_as(PV), size, len(sz), sz.ctypes.data_as(PV),
                                                      total + PAD, idx.ctypes.data_as(PV)))
    return idx, [int(x) for x in st]


def _rng_with_buffered_half(seed):
    """A generator whose next 32-bit draw is the buffered high half (has_uint32 = 1)."""
    rng = np.random.default_rng(seed)
    for _ in range(64):
        if rng.bit_generator.state["has_uint32"] == 1:
            return rng
        rng.integers(0, 7, size=1)
    raise AssertionError("no state with a buffered half-word")


# sizes beyond the shapes' own: zero tasks at the front, in the middle and at the end; more than one 64-lane round;
# a task above the fill level; single draws; 64 tasks
STREAM_SIZES = [s for _, s in tc.CASES] + [(0, 0, 5, 0, 130, 0), (1, 1, 1, 1), (65, 0, 64, 1), (200,), (0, 3),
                                           tuple([0, 2, 1, 0] * 16)]


@pytest.mark.parametrize("sizes", STREAM_SIZES, ids=lambda s: "_".join(map(str, s[:8])) + ("_x%d" % len(s) if len(s) > 8 else ""))
def test_index_kernel_matches_numpy(sizes):
    """Full and partly filled buffers (size above, between and below the task sizes, 1 and a size with many Lemire
    rejections), several seeds, from a fresh state and from one with has_uint32 = 1: indices, the untouched tail
    and the final generator state."""
    ran = 0
    for size in (64, 5, 1, 3 * (1 << 29)):  # 3 * 2^29: a quarter of all candidates is rejected
        for seed in (0, 1, 12345):
            for buffered in (False, True):
                rng = _rng_with_buffered_half(seed) if buffered else np.random.default_rng(seed)
                assert rng.bit_generator.state["has_uint32"] == int(buffered)
                before = _words(rng)
                want = np.concatenate(tc.task_indices(rng, sizes, size))
                idx, after = _kernel_indices(before, size, sizes)
                where = (sizes, size, seed, buffered)
                assert np.array_equal(idx[:len(want)], want), where
                assert (idx[len(want):] == -1).all(), ("a store past the batch", where)
                assert after == _words(rng), ("generator state", where)
                ran += 1
    assert ran == 24


def test_index_kernel_refuses_bad_sizes():
    from mtrl_amd import _lib as L

    st, idx = np.zeros(6, np.uint64), np.zeros(16, np.int32)
    for sizes in ((-1, 5), (0, 0), (17,), (9, 9)):
        sz = np.array(sizes, np.int32)
        assert L.load().mtsac_debug_replay_indices_tasks(st.ctypes.data_as(PV), 10, len(sz), sz.ctypes.data_as(PV), 16,
                                                         idx.ctypes.data_as(PV)) == -22, sizes


# ------------------------------------------------------------------ the gather alone, with planes
def _p(a):
    return None if a is None else a.ctypes.data_as(PV)


@pytest.mark.parametrize("name,sizes", tc.CASES, ids=tc.CASE_IDS)
def test_gather_kernel_task_major(name, sizes):
    """replay_gather_tasks between guard bands: fp32 rows, split3 and split2h planes, task ids, raw rewards."""
    from mtrl_amd import _lib as L

    T, n, W, A, E = tc.SHAPES[name]
    D, B, cap = 39 + T, n * T, 29
    store = tc.make_store(T, A, cap, seed=3)
    obs, nobs, act, rew, done = store
    R = RR.record_width(D, A)
    rec = RR.pack_records(obs.reshape(cap * T, D), act.reshape(cap * T, A), rew.reshape(-1), done.reshape(-1),
                          nobs.reshape(cap * T, D), R, pad=np.nan).reshape(cap, T, R)
    idx_t = tc.task_indices(np.random.default_rng(5), sizes, cap)
    idx = np.concatenate(idx_t).astype(np.int32)
    task = np.repeat(np.arange(T), sizes)
    rows = [x[idx, task] for x in (obs, act, nobs, done, rew)]
    ld_a, ld_c = D + 3, A + D + 5
    pa_ld, pc_ld = (D + 7) // 8 * 8, (A + D + 7) // 8 * 8 + 8
    pa_next, pa_rows, pc_rows = B + 3, 2 * B + 5, B + 2
    for plane_mode, in_max in ((0, None), (1, None), (2, 0.3), (2, 37.5)):
        np_ = 2 if plane_mode == 2 else 3
        dims = np.array([2, n, T, cap, D, A, T, 0, ld_a, ld_c, plane_mode, pa_ld, pc_ld, pa_next, pa_rows, pc_rows, R]
                        + list(sizes), np.int32)
        o = dict(xa=np.zeros((B, ld_a), np.float32), xa_next=np.zeros((B, ld_a), np.float32),
                 xc=np.zeros((B, ld_c), np.float32), xc_next=np.zeros((B, ld_c), np.float32),
                 xc_pi=np.zeros((B, ld_c), np.float32), rew=np.zeros(B, np.float32), done=np.zeros(B, np.float32),
                 task=np.zeros(B, np.int32), err=np.zeros(1, np.int32))
        if plane_mode:
            o["pa"] = np.zeros((np_, pa_rows, pa_ld), np.uint16)
            for k in ("pc", "pcn", "pcp"):
                o[k] = np.zeros((np_, pc_rows, pc_ld), np.uint16)
        e = np.full(1, -777, np.int32)
        im = None if in_max is None else np.array([in_max], np.float32)
        L.check(L.load().mtsac_debug_replay_gather(
            _p(dims), _p(rec), _p(idx), None, None, None, None, None, None, None, 0.0, _p(im), _p(o["xa"]),
            _p(o["xa_next"]), _p(o["xc"]), _p(o["xc_next"]), _p(o["xc_pi"]), _p(o["rew"]), _p(o["done"]), _p(o["task"]),
            _p(o["err"]), _p(o.get("pa")), _p(o.get("pc")), _p(o.get("pcn")), _p(o.get("pcp")),
            _p(e) if plane_mode == 2 else None))
        want = RR.gather_model(*rows, T, T, 0, ld_a, ld_c, plane_mode, pa_ld, pc_ld, pa_next, pa_rows, pc_rows, in_max)
        assert want["err"] == 0 and np.array_equal(want["task"], task)
        assert int(o["err"][0]) == 0
        if plane_mode == 2:
            assert int(e[0]) == want["e"]
        for k, w in want.items():
            if k in ("err", "e"):
                continue
            g = o[k]
            if k in ("pa", "pc", "pcn", "pcp"):  # the sign of a zero plane word is not part of the format
                g, w = np.where(g == 0x8000, 0, g).astype(np.uint16), np.where(w == 0x8000, 0, w).astype(np.uint16)
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype)
            assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), \
                (name, sizes, plane_mode, k)
    # a record whose one-hot names another task than its slot's: the row is flagged
    bad = rec.copy()
    t0 = int(task[0])
    if T > 1:
        bad[idx[0], t0, 39:39 + T] = 0
        bad[idx[0], t0, 39 + (t0 + 1) % T] = 1
        bad[idx[0], t0, D + A + 2 + 39:D + A + 2 + 39 + T] = bad[idx[0], t0, 39:39 + T]
        dims = np.array([2, n, T, cap, D, A, T, 0, ld_a, ld_c, 0, 0, 0, 0, 0, 0, R] + list(sizes), np.int32)
        err = np.zeros(1, np.int32)
        L.check(L.load().mtsac_debug_replay_gather(
            _p(dims), _p(bad), _p(idx), None, None, None, None, None, None, None, 0.0, None, _p(o["xa"]),
            _p(o["xa_next"]), _p(o["xc"]), _p(o["xc_next"]), _p(o["xc_pi"]), _p(o["rew"]), _p(o["done"]), _p(o["task"]),
            _p(err), None, None, None, None, None))
        assert int(err[0]) == 1


# ------------------------------------------------------------------ through the engine
def _engine(name, precision=0, normalize_rewards=0, **kw):
    from mtrl_amd.engine import MTSACEngine, make_config

    T, n, W, A, E = tc.SHAPES[name]
    c = make_config(precision=precision, num_tasks=T, task_count=T, obs_dim=39 + T, action_dim=A, actor_width=W,
                    critic_width=W, num_critics=E, batch_per_task=n, capacity=tc.CAPACITY,
                    normalize_rewards=normalize_rewards, **kw)
    e = MTSACEngine(c)
    e.enable_graph(False)
    return e


def _assert_sample(got, want_idx, want_rows):
    idx, (obs, act, nobs, done, rew) = got
    w_obs, w_act, w_nobs, w_done, w_rew, _ = want_rows
    np.testing.assert_array_equal(idx, np.concatenate(want_idx))
    for g, w in ((obs, w_obs), (act, w_act), (nobs, w_nobs), (done, w_done), (rew, w_rew)):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("name,sizes", tc.CASES, ids=tc.CASE_IDS)
def test_engine_sample_matches_numpy(name, sizes):
    """mtsac_sample under per-task sizes from a full and a partly filled buffer (a size above the fill level draws
    below the size), balanced draws before and after on the same stream, the generator state after every call, at
    every precision (the fp32 rows the sample returns do not depend on it), rewards raw under normalize_rewards."""
    T, n, W, A, E = tc.SHAPES[name]
    B = n * T
    store = tc.make_store(T, A, tc.CAPACITY, seed=2)
    for precision, norm, slots in ((0, 0, None), (1, 1, 5), (3, 2, None), (0, 1, None)):
        eng = _engine(name, precision, norm)
        tc.fill_engine(eng, store, slots)
        size = tc.CAPACITY if slots is None else slots
        if norm:  # statistics that would change every reward if they were applied
            eng.set_reward_stats(np.full(T, -3.0), np.full(T, 17.0))
        rng = np.random.default_rng(21)
        eng.seed_rng(21)
        # a balanced draw first: interleaved rows, n indices (it leaves has_uint32 as numpy does)
        want_i = rng.integers(0, max(size, n), size=n)
        idx, rows = eng.sample()
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(rows[0], store[0][want_i].reshape(B, -1))
        assert eng.get_rng_state() == rng.bit_generator.state
        assert not eng.task_batch_sizes_set() and eng.task_batch_sizes().tolist() == [n] * T
        # two uneven draws
        eng.set_task_batch_sizes(np.array(sizes))
        assert eng.task_batch_sizes_set() and eng.task_batch_sizes().tolist() == list(sizes)
        for _ in range(2):
            want_idx, want_rows = tc.reference_sample(store, rng, sizes, size, B)
            _assert_sample(eng.sample(), want_idx, want_rows)
            assert eng.get_rng_state() == rng.bit_generator.state
        # back to balanced on the same stream
        eng.set_task_batch_sizes(None)
        want_i = rng.integers(0, max(size, n), size=n)
        idx, rows = eng.sample()
        np.testing.assert_array_equal(idx, want_i)
        if norm == 0:
            np.testing.assert_array_equal(rows[4], store[3][want_i].reshape(B, 1))
        else:  # the int branch normalises
            assert not np.array_equal(rows[4], store[3][want_i].reshape(B, 1))
        assert eng.get_rng_state() == rng.bit_generator.state
        eng.close()


def test_engine_sample_from_a_buffered_half_word():
    name, sizes = "t3", (1, 0, 23)
    T, n, W, A, E = tc.SHAPES[name]
    store = tc.make_store(T, A, tc.CAPACITY, seed=4)
    eng = _engine(name)
    tc.fill_engine(eng, store)
    rng = _rng_with_buffered_half(9)
    eng.set_rng_state(rng.bit_generator.state)
    eng.set_task_batch_sizes(sizes)
    want_idx, want_rows = tc.reference_sample(store, rng, sizes, tc.CAPACITY, n * T)
    _assert_sample(eng.sample(), want_idx, want_rows)
    assert eng.get_rng_state() == rng.bit_generator.state
    eng.close()


def test_error_codes():
    from mtrl_amd import _lib as L
    from mtrl_amd.engine import MTSACEngine, make_config

    name = "t3"
    T, n, W, A, E = tc.SHAPES[name]
    eng = _engine(name)
    with pytest.raises(L.MTSACError, match="-22"):
        eng.set_task_batch_sizes(np.array([9, 8, 8]))  # bad sum
    with pytest.raises(L.MTSACError, match="-22"):
        eng.set_task_batch_sizes(np.array([-1, 17, 8]))  # negative
    with pytest.raises(ValueError):
        eng.set_task_batch_sizes(np.array([12, 12]))  # wrong length, before the library is called
    with pytest.raises(ValueError):
        eng.set_task_batch_sizes(np.array([8.0, 8.0, 8.0]))
    assert not eng.task_batch_sizes_set()
    with pytest.raises(L.MTSACError, match="-22"):
        eng.task_losses()  # logging was never on
    # surgery on: the sizes are refused; sizes set: the surgery setters are refused (-95 both ways)
    for on in (lambda: eng.set_pcgrad(True), lambda: eng.set_cagrad(True), lambda: eng.set_gradnorm(True)):
        on()
        with pytest.raises(L.MTSACError, match="-95"):
            eng.set_task_batch_sizes(np.array([9, 8, 7]))
        eng.set_pcgrad(False), eng.set_cagrad(False), eng.set_gradnorm(False)
    eng.set_task_batch_sizes(np.array([9, 8, 7]))
    for on in (lambda: eng.set_pcgrad(True), lambda: eng.set_cagrad(True), lambda: eng.set_gradnorm(True)):
        with pytest.raises(L.MTSACError, match="-95"):
            on()
    eng.set_task_batch_sizes(None)
    eng.set_pcgrad(True)
    eng.set_pcgrad(False)
    eng.close()
    # a size above the buffer's slots per task would index past the store
    small = MTSACEngine(make_config(num_tasks=3, task_count=3, obs_dim=42, actor_width=36, critic_width=36,
                                    batch_per_task=8, capacity=16))
    with pytest.raises(L.MTSACError, match="-22"):
        small.set_task_batch_sizes(np.array([24, 0, 0]))
    small.set_task_batch_sizes(np.array([16, 8, 0]))
    small.close()
    # a task-sharded engine
    shard = MTSACEngine(make_config(num_tasks=4, task_begin=0, task_count=2, obs_dim=43, actor_width=36, critic_width=36,
                                    batch_per_task=4, capacity=16))
    with pytest.raises(L.MTSACError, match="-95"):
        shard.set_task_batch_sizes(np.array([5, 3]))
    shard.set_task_batch_sizes(None)  # clearing what is not set is fine
    shard.close()
    # a collective hook on an unsharded engine makes it a shard of a group
    hooked = _engine(name)
    hooked.set_allreduce_hook(lambda ptr, count: None)
    with pytest.raises(L.MTSACError, match="-95"):
        hooked.set_task_batch_sizes(np.array([9, 8, 7]))
    hooked.close()
