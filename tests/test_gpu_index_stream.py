"""replay_indices_kernel (mtrl_amd/csrc/replay.hip) alone, through mtsac_debug_replay_indices, against
oracle.pcg64.PCG64State (itself pinned to numpy at the same cases by tests/test_index_stream_cpu.py, which also
asserts that the cases reach the Lemire rejection branch: a rejected buffered half-word, a last draw from either
half, three and more rounds, hundreds of rejections).  Per case three consecutive calls on one state; after each,
idx[:n] and the six state words equal the reference's and idx[n:] is untouched (-1 between guard bands)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import index_stream_cases as IC

pytestmark = pytest.mark.gpu

PAD = 70  # idx entries past n: more than one round's worth of lanes


def _run(state, mode, high_or_size, n):
    from mtrl_amd import _lib as L

    st = np.array(state, np.uint64)
    idx = np.zeros(n + PAD, np.int32)
    L.check(L.load().mtsac_debug_replay_indices(st.ctypes.data_as(ctypes.c_void_p), mode, high_or_size, n, n + PAD,
                                                idx.ctypes.data_as(ctypes.c_void_p)))
    return idx, [int(x) for x in st]


@pytest.mark.parametrize("high", IC.HIGHS)
def test_index_stream_matches_reference(high):
    for seed in IC.SEEDS:
        for n in IC.NS:
            state = None
            for call, (before, want, after, ev) in enumerate(IC.reference(seed, high, n)):
                state = before if state is None else state
                assert state == before  # the device's state feeds the next call
                idx, state = _run(state, 0, high, n)
                where = (seed, high, n, call, ev)
                assert np.array_equal(idx[:n], want), where
                assert (idx[n:] == -1).all(), ("a store at a position >= n", where)
                assert state == after, ("generator state", where)
                if high == 1:
                    assert (idx[:n] == 0).all() and state == before


def test_buffer_size_mode_draws_below_max_of_size_and_n():
    """replay_indices reads *buf_size on the device: high = max(size, n) (sizes below, at and above n)."""
    from oracle.pcg64 import PCG64State

    for n, size in ((65, 1), (65, 64), (65, 65), (65, 66), (129, 1000000), (1, 1), (2, 1)):
        s = PCG64State.from_seed(11)
        s.integers(7, 1)  # enter with a buffered half-word
        before = IC.state_words(s)
        want = s.integers(max(size, n), n)
        idx, state = _run(before, 1, size, n)
        assert np.array_equal(idx[:n], want) and (idx[n:] == -1).all(), (n, size)
        assert state == IC.state_words(s), (n, size)


def test_high_out_of_range_is_refused():
    from mtrl_amd import _lib as L

    st, idx = np.zeros(6, np.uint64), np.zeros(8, np.int32)
    for high in (1 << 31, 1 << 32, 0):
        assert L.load().mtsac_debug_replay_indices(st.ctypes.data_as(ctypes.c_void_p), 0, high, 4, 8,
                                                   idx.ctypes.data_as(ctypes.c_void_p)) == -22
