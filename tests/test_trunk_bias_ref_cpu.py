"""The numpy reference of the trunk bias-grad and layout tests (tests/trunk_bias_ref.py) checked on its own: the
plane formats, the fragment layout, the chunked sums, the launcher replicas, and the condition that makes the
GPU tolerances worth asserting -- a single dropped row must show."""

from __future__ import annotations

import numpy as np
import pytest

import trunk_bias_ref as R


@pytest.mark.parametrize("N,ldk", [(16, 32), (48, 64), (400, 416), (2048, 96)])
def test_frag_off_is_a_bijection(N, ldk):
    n, k = np.meshgrid(np.arange(N), np.arange(ldk), indexing="ij")
    off = R.frag_off(n, k, ldk).ravel()
    assert off.min() == 0 and off.max() == N * ldk - 1
    assert np.unique(off).size == N * ldk
    # every 16-row x 32-k fragment is 512 contiguous elements, 8 k of one row together
    assert np.array_equal(np.sort(off.reshape(N, ldk)[:16, :32].ravel()), np.arange(512))
    assert np.array_equal(np.diff(off.reshape(N, ldk)[3, 8:16]), np.ones(7, np.int64))


def _values(rng, n):
    x = rng.standard_normal(n).astype(np.float32) * (10.0 ** rng.uniform(-12, 6, n)).astype(np.float32)
    x[:8] = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 1e-33, 65504.0]  # (exact down to ~2^-110: bf16 subnormals are coarse)
    return x


def test_split3_planes_sum_back_exactly():
    x = _values(np.random.default_rng(1), 20000)
    h, m, l = R.split3(x)
    for p in (h, m, l):  # each plane is a bf16 value
        assert np.array_equal(p.view(np.uint32) & 0xFFFF, np.zeros(p.size, np.uint32))
    back = (h.astype(np.float64) + m.astype(np.float64)) + l.astype(np.float64)
    assert np.array_equal(back.astype(np.float32), x)
    assert np.array_equal(((h + m) + l).astype(np.float32), x)  # and in float32, the order debug.cpp adds them in
    assert np.array_equal(R.bf16_words(h).view(np.int16) > 0, x > 0)  # the mask the bf16 high plane gives


@pytest.mark.parametrize("e", [-20, 0, 14])
def test_split2h_planes_reproduce_positive(e):
    rng = np.random.default_rng(22 + e)
    top = np.float32(2.0 ** (15 - e))
    x = (rng.standard_normal(20000) * top / 4).astype(np.float32)
    x = np.clip(x, -top * np.float32(0.999), top * np.float32(0.999))
    x[:10] = [0.0, -0.0, 1e-30, -1e-30, 1e-37, top * np.float32(1 - 2.0 ** -12), -top * np.float32(1 - 2.0 ** -12),
              top * np.float32(2.0 ** -30), -top * np.float32(2.0 ** -30), top * np.float32(2.0 ** -40)]
    hw, lw = R.split2h(x, e)
    # the mask is a ReLU output: for x >= 0 the planes give 'x > 0' exactly (a negative x may carry a positive l)
    nn = ~np.signbit(x)
    assert np.array_equal(R.split2h_positive(hw, lw)[nn], x[nn] > 0)
    assert not R.split2h_positive(hw, lw)[1] and not R.split2h_positive(hw, lw)[3]  # -0.0, -1e-30
    assert np.isfinite(hw.view(np.float16)).all() and np.isfinite(lw.view(np.float16)).all()
    # 22 bits above 2^-3 of the range, 2^-24 of the scaled unit below (the sticky subnormal included)
    err = np.abs(R.split2h_value(hw, lw, e) - x.astype(np.float64))
    assert np.all(err <= 2.0 ** -21 * np.abs(x) + 1.01 * 2.0 ** (-24 - e))


def test_plane_exp_keeps_the_bound_in_range():
    for b in (1e-20, 1e-6, 0.9999, 1.0, 3.7, 255.9, 32768.0, 1e20):
        e = R.plane_exp(b)
        assert b * 2.0 ** e < 2.0 ** 15 and b * 2.0 ** e >= 2.0 ** 13, (b, e)
    assert R.plane_exp(0.0) == 0 and R.plane_exp(float("inf")) == 0


def test_split_planes_zero_fill_and_untouched():
    x = np.arange(1, 1 + 3 * 5, dtype=np.float32).reshape(1, 3, 5)
    w = R.split_planes(x, out_rows=4, out_cols=8, ldo=12, arows=6).reshape(1, 3, 6, 12)
    assert np.array_equal(w[0, 0, :3, :5], R.bf16_words(x[0]))
    assert (w[0, :, :4, 5:8] == 0).all() and (w[0, :, 3, :8] == 0).all()  # zero fill inside [out_rows][out_cols]
    assert (w[0, :, 4:, :] == R.UNTOUCHED).all() and (w[0, :, :, 8:] == R.UNTOUCHED).all()
    t = R.split_planes(x, out_rows=5, out_cols=130, ldo=136, arows=5, transpose=True).reshape(1, 3, 5, 136)
    assert np.array_equal(t[0, 0, :, :3], R.bf16_words(x[0].T))
    assert (t[0, :, :, 3:64] == 0).all() and (t[0, :, :, 64:] == R.UNTOUCHED).all()  # past the source's tiles
    h = R.split_planes(x, out_rows=4, out_cols=8, ldo=8, arows=4, e2h=3).reshape(1, 3, 4, 8)
    assert (h[0, 2] == R.UNTOUCHED).all() and h[0, 0, 0, 0] == np.float16(8.0).view(np.uint16)


def test_chunked_colsum():
    X = np.random.default_rng(3).standard_normal((2, 37, 5))
    s, a = R.chunked_colsum(X, 16)
    assert s.shape == (2, 3, 5)
    assert np.allclose(s[:, 2], X[:, 32:].sum(axis=1)) and np.allclose(s.sum(axis=1), X.sum(axis=1))
    assert np.allclose(a[:, 0], np.abs(X[:, :16]).sum(axis=1))
    assert np.array_equal(R.tol_sum(1, a), np.zeros_like(a))  # one row: the sum is the value, exactly


def test_x3s_never_picks_ti_8():
    """TI = 8 always ties with or loses to TI = 4 (half the rows per tile, at most twice the tiles, so at most
    twice the rounds) and ties go to the smaller tile: every other height is reachable."""
    got = {R.x3s_ti(M, N, E) for M in range(1, 7000, 7) for N in (8, 60, 400, 2048) for E in (1, 2)}
    assert got == {4, 5, 6, 7}
    for M, N, E in [(100000, 2048, 2), (128, 64, 1), (1 << 20, 4096, 8)]:
        assert R.x3s_ti(M, N, E) != 8


def test_launcher_replicas_on_known_shapes():
    assert R.bf16_bm(6400, 2048, 2) == 400 and R.bf16_bm(6400, 2048, 1) == 208
    assert R.bf16_bm(1280, 2048, 2) == 80 and R.bf16_bm(1270, 2040, 1) == 48
    assert R.split_plan(896, 2048, 2048, 2) == (128, 2)  # 896 rows: 7 x 128, two slices instead of three
    assert R.split_plan(6400, 2048, 2048, 1) == (208, 1)
    assert R.x3f_plan(416, 256, 64, 1, "split3", False, False) is None  # too few workgroups


def test_sum_bar_accepts_any_order_and_rejects_a_dropped_row():
    """tol_sum against a launch's own fp32 C: float32 sums of a chunk in three different orders pass, the same sum
    with the chunk's last live row left out fails in nearly every column."""
    r, N = 208, 512
    A, B, _, mask = R.make_case(1, r, N, 64, seed=5)
    C = np.where(mask > 0, R.gemm_ref(A, B)[0], 0.0).astype(np.float32)[0]
    s, sa = R.chunked_colsum(C[None].astype(np.float64), r)
    tol = R.tol_sum(r, sa)[0, 0]
    fwd = np.zeros(N, np.float32)
    for i in range(r):
        fwd += C[i]
    rev = np.zeros(N, np.float32)
    for i in reversed(range(r)):
        rev += C[i]
    tree = C.reshape(8, 26, N).sum(axis=1, dtype=np.float32).sum(axis=0, dtype=np.float32)
    for got in (fwd, rev, tree):
        assert np.all(np.abs(got.astype(np.float64) - s[0, 0]) <= tol)
    short = fwd - C[r - 1]
    live = mask[0, r - 1] > 0
    assert np.mean(np.abs(short.astype(np.float64) - s[0, 0])[live] > tol[live]) >= 0.99


# (rows per chunk, K, precision) of the widest GPU cases of each family: the unsplit 208-row tile, the bf16
# 400-row tile, the finishing pass's 16 rows at three slices, gemm_x3s at TI = 7 and on the padded width (TI = 5)
@pytest.mark.parametrize("r,K,k_live,bf16", [(208, 64, None, False), (400, 64, None, True), (16, 1024, 1000, False),
                                             (112, 64, None, False), (80, 416, 400, True)])
def test_one_dropped_row_shows(r, K, k_live, bf16):
    """The sensitivity condition: on make_case's operands, leaving any one row out of a chunk's column sum moves
    the reference past the planes-only tolerance (the widest one used) in >= 95 % of that row's unmasked columns.
    Were it not so the tolerance would hide a kernel that skips a row."""
    E, M, N = 1, 2 * r, 256
    A, B, _, mask = R.make_case(E, M, N, K, seed=r + K, k_live=k_live)
    if bf16:
        A, B = R.bf16_rne(A), R.bf16_rne(B)
    acc, scale = R.gemm_ref(A, B)
    want = np.where(mask > 0, acc, 0.0)
    _, sabs = R.chunked_colsum(np.abs(want), r)
    sscale, _ = R.chunked_colsum(np.where(mask > 0, scale, 0.0), r)
    tol = R.GEMM_REL * sscale + R.tol_sum(r, sabs)
    worst = R.sensitivity(want, mask > 0, tol, r)
    print("least fraction of columns in which a dropped row shows:", worst)
    assert worst >= 0.95
