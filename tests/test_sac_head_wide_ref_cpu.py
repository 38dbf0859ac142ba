"""What the bars of tests/sac_head_wide_bounds.py accept and reject, without a GPU: a float32 numpy evaluation
of each wide head kernel in the order heads_wide.h documents lies inside them, and four seeded mistakes (a
dropped row, two swapped output columns, a missing ReLU mask, the neighbouring task's head) lie outside."""

from __future__ import annotations

import numpy as np
import pytest

import sac_head_cases as C
import sac_head_ref as R
import sac_head_wide_bounds as Wb

f32, f64 = np.float32, np.float64
CASES = [(5, 36, (15, 16, 17)), (8, 4, (3, 0, 33)), (19, 260, (5, 17)), (64, 20, (33,))]


def test_constants_follow_the_documented_orders():
    assert Wb.k_order(20, 0) == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    assert Wb.k_order(20, 1) == [16, 17, 18, 19] and Wb.k_order(20, 2) == []
    assert sorted(k for g in range(Wb.KS) for k in Wb.k_order(516, g)) == list(range(516))
    assert Wb.chain_len(516) == 8 * 16 + 4 == len(Wb.k_order(516, 0)) and Wb.chain_len(4) == 4
    assert Wb.c_dot_wide(516) == 136 and Wb.c_dz_wide(128) == 128 and Wb.c_agrad_wide(516, 4) == 531
    assert [Wb.c_slice_wide(n) for n in (1, 16, 64, 65, 257)] == [5, 5, 5, 6, 9]
    assert Wb.c_colsum_wide(257, 5) == 29 and Wb.c_wgrad_wide(257) == 257 and Wb.c_bgrad_wide(0) == 1


@pytest.mark.parametrize("A,W,counts", CASES)
def test_policy_bars(A, W, counts):
    c = C.policy_case(A, W, counts)
    r, bnd, _ = Wb.policy_expect(c, 0)
    task, hd = c["task"], 2 * A
    out = Wb.head_out_f32(c["h"][0], c["Wh"], c["bh"], task)
    assert R.within(out, r["out"], bnd["out"]), R.worst(out, r["out"], bnd["out"])
    # two output columns swapped in one ordinary row
    row = int(np.flatnonzero(c["h"][0].sum(1) > 1.5)[0])
    bad = out.copy()
    bad[row, [1, A + 1]] = bad[row, [A + 1, 1]]
    assert not R.within(bad, r["out"], bnd["out"])
    # the neighbouring task's head (cases with one task: its kernel rolled by one row)
    other = (task + 1) % c["T_l"] if c["T_l"] > 1 else task
    Wh = c["Wh"] if c["T_l"] > 1 else np.roll(c["Wh"], 1, axis=1)
    assert not R.within(Wb.head_out_f32(c["h"][0], Wh, c["bh"], other), r["out"], bnd["out"])


@pytest.mark.parametrize("A,W,counts", CASES)
def test_backward_bars(A, W, counts):
    hd = 2 * A
    c = C.backward_case(hd, 1, W, counts)
    want, bnd, _ = Wb.backward_expect(c)
    task, T_l = c["task"], c["T_l"]
    h, Wh, dout = c["h"][0], c["Wh"][0], c["dout"][0]
    got = Wb.backward_f32(h, Wh, dout, task, T_l)
    for k in ("dz", "dbp", "dWh", "dbh"):
        assert R.within(got[k][None], want[k], bnd[k]), (k, R.worst(got[k][None], want[k], bnd[k]))
    # no ReLU mask
    nomask = Wb.backward_f32(np.ones_like(h), Wh, dout, task, T_l)["dz"]
    assert not R.within(nomask[None], want["dz"], bnd["dz"])
    # one row dropped from the sums (a row with a non-zero dout)
    drop = int(np.flatnonzero(np.abs(dout).sum(1) > 0)[-1])
    keep = np.arange(len(task)) != drop
    less = Wb.backward_f32(h[keep], Wh, dout[keep], task[keep], T_l)
    for k in ("dbp", "dWh", "dbh"):
        assert not R.within(less[k][None], want[k], bnd[k]), k


@pytest.mark.parametrize("A,E,Wc,B", [(19, 2, 36, 17), (33, 1, 260, 5), (64, 4, 20, 33)])
def test_action_grad_bars(A, E, Wc, B):
    c = C.action_grad_case(A, E, Wc, B)
    r, bnd = Wb.action_grad_expect(c, False)
    ga = Wb.action_grad_f32(c["dz1"], c["W0"], A)
    assert R.within(ga, r["g_crit"], bnd["ga"]), R.worst(ga, r["g_crit"], bnd["ga"])
    bad = ga.copy()
    row = int(np.flatnonzero(np.abs(c["dz1"]).sum((0, 2)) > 0)[0])
    bad[row, [0, 1]] = bad[row, [1, 0]]
    assert not R.within(bad, r["g_crit"], bnd["ga"])
    if E > 1:  # a member dropped from the chain
        one = Wb.action_grad_f32(c["dz1"][:1], c["W0"][:1], A)
        assert not R.within(one, r["g_crit"], bnd["ga"])
