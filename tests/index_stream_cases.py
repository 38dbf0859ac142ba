"""The index-stream cases shared by tests/test_index_stream_cpu.py (the reference against numpy, and that the list
reaches the Lemire rejection branch in every way that matters) and tests/test_gpu_index_stream.py (the kernel
against the reference).  A case is (seed, high, n): three consecutive calls on one state, so a call is entered
with and without a buffered half-word.

high = 3 << 29 and 2^30 + 1 reject a candidate with probability (2^32 mod high) / 2^32 = 1/4, 2^31 - 1 with
2 / 2^32, 100000 with 1.6e-5; 3, 2 and 1 are the smallest ranges (1 draws nothing).  n = 63 .. 65 and 127 .. 129
sit on both sides of one and two rounds of the kernel's 128 candidates; 1000 needs eight or more."""

from __future__ import annotations

import functools

import numpy as np

from oracle.pcg64 import MASK32, PCG64State

SEEDS = (0, 7)
HIGHS = (3 << 29, (1 << 30) + 1, (1 << 31) - 1, 100000, 3, 2, 1)
NS = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
CALLS = 3
STATE_WORDS = 6


class TracedPCG64(PCG64State):
    """PCG64State that records where every 32-bit word of a call came from: 'buf' (the high half an earlier call
    left buffered), 'lo' / 'hi' (the halves of a 64-bit word drawn in this call)."""

    __slots__ = ("trace", "fresh")

    def begin(self):
        self.trace, self.fresh = [], False

    def next32(self):
        if self.has_uint32:
            self.trace.append("hi" if self.fresh else "buf")
        else:
            self.trace.append("lo")
            self.fresh = True
        return super().next32()


def state_words(s: PCG64State):
    return [s.state >> 64, s.state & ((1 << 64) - 1), s.inc >> 64, s.inc & ((1 << 64) - 1), s.has_uint32, s.uinteger & MASK32]


def traced_call(s: TracedPCG64, high: int, n: int):
    """One integers(0, high, n) call: (idx, state words after, events)."""
    s.begin()
    entered_buffered = bool(s.has_uint32)
    idx, first_draw_words = np.zeros(n, np.int64), 0
    for i in range(n):
        before = len(s.trace)
        idx[i] = s.bounded(high)
        if i == 0:
            first_draw_words = len(s.trace) - before
    ev = dict(
        rejections=len(s.trace) - (n if high > 1 else 0),
        buffered_rejected=entered_buffered and high > 1 and s.trace[0] == "buf" and first_draw_words > 1,
        last=s.trace[-1] if s.trace else None,
        rounds=-(-sum(1 for w in s.trace if w == "lo") // 64),  # 64 lanes draw one 64-bit word each per round
    )
    return idx, state_words(s), ev


@functools.lru_cache(maxsize=None)
def reference(seed: int, high: int, n: int):
    """[(state words before, idx, state words after, events)] of the CALLS calls of one case (computed once)."""
    base = PCG64State.from_seed(seed)
    s = TracedPCG64(base.state, base.inc, base.has_uint32, base.uinteger)
    out = []
    for _ in range(CALLS):
        before = state_words(s)
        idx, after, ev = traced_call(s, high, n)
        out.append((before, idx, after, ev))
    return out


def all_cases():
    return [(seed, high, n) for seed in SEEDS for high in HIGHS for n in NS]
