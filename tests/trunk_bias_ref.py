"""Plain numpy statements of what the trunk GEMMs' bias-grad path and the layout kernels compute
(mtrl_amd/csrc/gemm_x3f*.hip, gemm_x3s.hip, gemm_x3p.hip, layout.hip, gemm_common.h): the plane formats bit for
bit, the chunked column sums in float64, the launchers' row-tile choices, and the tolerances the GPU tests hold
the kernels to.  No float32 arithmetic except where the format itself is float32 (the split residuals).

Tolerances (U = 2^-24, float32 round to nearest; none is a measured number)
---------------------------------------------------------------------------
 * `tol_sum(r, S)`: r float32 values added in ANY order lie within (r - 1) U S of their exact sum, S the sum of
   their magnitudes (r - 1 additions, each rounding once, first order in U).  Used for a chunk's column sums
   against the launch's own fp32 C (r = rows in the chunk) and for db against dbp (r = chunks).
 * `GEMM_REL` = 4e-6: the plane GEMM tests' bound |C - exact| <= 4e-6 sum_k |a b| (+ |bias| for bias+ReLU), what
   an fp32 GEMM with fp32 accumulation meets at these K.  Where the launch returns no fp32 C (planes only) a
   chunk's column sum is held to the sum over its rows of that bound plus `tol_sum` on the exact |C|.
 * split2h output planes carry C to 22 bits: |planes - C| <= 2^-21 |C| + 1.01 2^(-24 - e) (test_gpu_x3f.py).

Sensitivity: with the Gaussian operands of `make_case`, dropping one row from a chunk's sum moves it by |C_ij|
~ |N(0, 1)|, far above these bars: `sensitivity` measures how often.
"""

from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
GEMM_REL = 4e-6
UNTOUCHED = 0xFFFF  # the 16-bit word of a plane element no kernel wrote (guarded outputs start as all-ones)


# ------------------------------------------------------------------ plane formats
def bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_words(x: np.ndarray) -> np.ndarray:
    """The 16-bit words of bf16-representable float32 values."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def split3(x: np.ndarray):
    """split3_dev: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m), the residuals in float32."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_rne(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_rne(r1)
    l = bf16_rne((r1 - m).astype(np.float32))
    return h, m, l


def split2h(x: np.ndarray, e: int):
    """split2h_dev at exponent e, as fp16 words: h = fp16(x 2^e), l = fp16(x 2^e - h); a positive x whose planes
    both round to zero keeps the smallest subnormal in l (the sticky subnormal)."""
    x = np.ascontiguousarray(x, np.float32)
    y = (x * np.float32(2.0 ** e)).astype(np.float32)
    h = y.astype(np.float16)
    l = (y - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    hw, lw = h.view(np.uint16).copy(), l.view(np.uint16).copy()
    lw[(x > 0) & (h == 0) & (l == 0)] = 1
    return hw, lw


def split2h_value(hw: np.ndarray, lw: np.ndarray, e: int) -> np.ndarray:
    return (hw.view(np.float16).astype(np.float64) + lw.view(np.float16).astype(np.float64)) * 2.0 ** -e


def split2h_positive(hw: np.ndarray, lw: np.ndarray) -> np.ndarray:
    """The ReLU mask the data grad reads from fp16 planes: h > 0 or l > 0 as signed 16-bit words."""
    return (hw.view(np.int16) > 0) | (lw.view(np.int16) > 0)


def plane_exp(bound: float) -> int:
    """gemm_common.h plane_exp: the exponent e with bound 2^e < 2^15, a 2^-8 margin on the float32 bound."""
    b = np.float32(np.float32(bound) * np.float32(1.00390625))
    if not (b > 0) or not (b < np.float32(3.0e38)):
        return 0
    return min(100, max(-100, 15 - math.frexp(float(b))[1]))


def frag_off(n, k, ldk):
    """gemm_common.h frag_off: element (n, k) of a plane [rows][ldk] in the fragment layout."""
    n, k = np.asarray(n, np.int64), np.asarray(k, np.int64)
    return (((n >> 4) * (ldk >> 5) + (k >> 5)) << 9) + (((n & 15) + 16 * ((k >> 3) & 3)) << 3) + (k & 7)


def split_planes(x, out_rows, out_cols, ldo, arows, transpose=False, frag=False, e2h=None):
    """split_planes on x [batch][rows][cols] (the source's own padding already cut off): the 16-bit words
    [batch][3][arows * ldo], UNTOUCHED where the launch writes nothing.  The row form (not transposed, out_cols,
    ldo and the plane stride multiples of 4) writes all of [out_rows][out_cols], zeros past the source; the
    64 x 64 tile form's grid covers the source's tiles only, so it writes the part of [out_rows][out_cols] inside
    them and leaves the rest alone.  split2h (e2h an exponent) writes two planes."""
    x = np.ascontiguousarray(x, np.float32)
    batch, rows, cols = x.shape
    po = arows * ldo
    row_form = not transpose and out_cols % 4 == 0 and ldo % 4 == 0 and po % 4 == 0
    src = x.transpose(0, 2, 1) if transpose else x
    srows, scols = src.shape[1:]
    if row_form:
        wr, wc = out_rows, out_cols
    else:  # the tiles of the source, seen from the output
        up = lambda v: -(-v // 64) * 64
        wr, wc = min(out_rows, up(srows)), min(out_cols, up(scols))
    v = np.zeros((batch, wr, wc), np.float32)
    v[:, :min(wr, srows), :min(wc, scols)] = src[:, :min(wr, srows), :min(wc, scols)]
    if e2h is None:
        words = [bf16_words(p) for p in split3(v)]
    else:
        words = list(split2h(v, e2h))
    r, c = np.meshgrid(np.arange(wr), np.arange(wc), indexing="ij")
    off = frag_off(r, c, ldo) if frag else r * ldo + c
    out = np.full((batch, 3, po), UNTOUCHED, np.uint16)
    for q, w in enumerate(words):
        out[:, q, off.ravel()] = w.reshape(batch, -1)
    return out


# ------------------------------------------------------------------ column sums and tolerances
def chunked_colsum(X: np.ndarray, rows_per_chunk: int):
    """X [E][M][N] float64 -> (sums, sums of magnitudes), each [E][chunks][N], chunk c = rows [c r, (c + 1) r)."""
    E, M, N = X.shape
    chunks = -(-M // rows_per_chunk)
    pad = chunks * rows_per_chunk - M
    Xp = np.concatenate([X, np.zeros((E, pad, N))], axis=1) if pad else X
    Xp = Xp.reshape(E, chunks, rows_per_chunk, N)
    return Xp.sum(axis=2), np.abs(Xp).sum(axis=2)


def tol_sum(r: int, S):
    return (r - 1) * U * np.asarray(S, np.float64)


def sensitivity(C: np.ndarray, active: np.ndarray, tol: np.ndarray, rows_per_chunk: int) -> float:
    """The least, over the rows of C [E][M][N], of the fraction of the row's unmasked columns in which dropping
    that row from its chunk's sum moves the sum (by |C_ij|) past the chunk's tolerance tol [E][chunks][N]."""
    E, M, N = C.shape
    worst = 1.0
    for e in range(E):
        for i in range(M):
            on = active[e, i]
            if on.any():
                seen = np.abs(C[e, i, on]) > tol[e, i // rows_per_chunk, on]
                worst = min(worst, float(seen.mean()))
    return worst


def make_case(E, M, N, K, seed, k_live=None):
    """The Gaussian operands every GPU case runs on: A [E][M][K] ~ N(0, 1) (zero columns from k_live on: K a
    padded width), B [E][N][K] ~ N(0, 1 / K), bias ~ 0.1 N(0, 1), and a ReLU output as the mask with seven columns
    of 1e-30 (tiny activations still count as positive)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((E, M, K), dtype=np.float32)
    if k_live is not None:
        A[:, :, k_live:] = 0
    B = (rng.standard_normal((E, N, K), dtype=np.float32) / np.float32(math.sqrt(K))).astype(np.float32)
    bias = (rng.standard_normal((E, N), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    mask = np.maximum(rng.standard_normal((E, M, N), dtype=np.float32), 0)
    mask[:, :, :7] = 1e-30
    return A, B, bias, mask


def gemm_ref(A, B):
    """float64 A B^T per member and the sum of the products' magnitudes."""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    Bt = B64.transpose(0, 2, 1)
    return A64 @ Bt, np.abs(A64) @ np.abs(Bt)


# ------------------------------------------------------------------ the launchers' choices, restated
def x3s_ti(M, N, batch):
    """gemm_x3s_ti: rows per tile / 16, the fewest rounds of 256 workgroups x rows per tile, ties to the smaller."""
    best, bc = 4, None
    for ti in range(4, 9):
        tiles = -(-M // (16 * ti)) * -(-N // 64) * batch
        cost = -(-tiles // 256) * ti
        if bc is None or cost < bc:
            bc, best = cost, ti
    return best


def bf16_bm(M, N, batch):
    """gemm_x3f.hip bf16_bm: the row tile of the one-plane kernel."""
    ny = -(-N // 256)
    best, best_t = 208, 1e30
    for bm in (48, 80, 208, 400):
        rounds = -(-(-(-M // bm) * ny * batch) // 256)
        t = rounds * max(8.0 * bm, 4.57 * (bm + 256))
        if t < best_t - 1e-9:
            best_t, best = t, bm
    return best


def split_plan(M, N, K, batch):
    """gemm_x3f.hip split_plan: (row tile, K slices) of a launch allowed to split."""
    if -(-M // 208) * -(-N // 256) * batch >= 192:
        return 208, 1
    smax = min(8, max(1, K // 64 // 4))
    best, best_cost = (208, 1), 1e30
    for bm in (208, 128):
        tiles = -(-M // bm) * -(-N // 256) * batch
        work = 1.0 if bm == 208 else bm / 208 / 0.9
        for sp in range(1, smax + 1):
            cost = -(-tiles * sp // 256) * work / sp + 0.04 * (sp - 1)
            if cost < best_cost - 1e-9:
                best_cost, best = cost, (bm, sp)
    return best


FAMILIES = ("x3f", "x3f_split_fin", "x3f_split_pass", "x3s")


def x3f_plan(M, N, K, batch, prec, split, fin):
    """What gemm_x3f does with a bias+ReLU or mask16 launch that writes dbp (K a multiple of 64): (family index,
    rows per dbp chunk), or None where gemm_x3f_ok refuses it.  prec: 'split3', 'split2h' or 'bf16'."""
    bm, s = split_plan(M, N, K, batch)
    tiles = lambda b: -(-M // b) * -(-N // 256) * batch
    slices = 1
    if split and N % 4 == 0 and not (prec == "bf16" and tiles(bf16_bm(M, N, batch)) >= 128):
        slices = s
    if slices == 1:
        b = bf16_bm(M, N, batch) if prec == "bf16" else 208
        return (0, b) if tiles(b) >= 192 else None
    if tiles(bm) * slices < 192:
        return None
    fin_ok = fin and prec != "bf16" and (prec != "split2h" or s == 2) and tiles(bm) <= 4096
    return (1, bm) if fin_ok else (2, 16)
