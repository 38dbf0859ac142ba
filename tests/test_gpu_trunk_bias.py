"""The trunk GEMMs as the engine calls them, one launch family at a time against float64
(mtsac_debug_gemm_x3f_ld, mtsac_debug_wgrad_finish): padded plane strides (ld_n > N, rows_p > M), guarded
outputs that start as NaN, the bias grad's column-sum partials (SplitGemmParams::dbp) with the chunk count the
engine derives for the next weight grad, and the three launches that finish a bias grad from them.

Per data-grad case (ReLU mask from the activation's planes): the engine's planes-only form, then C + planes,
then bias+ReLU.  Asserted each time: the family and row tile that ran (info), dbp finite in chunks [0, chunks)
and NaN after them, dbp and db within the derived tolerances of tests/trunk_bias_ref.py, C and the planes
within the plane GEMM tests' bounds inside [M][N], every plane element in rows [M, rows_p) and columns
[N, ld_n) still NaN, no guard band written (the entry returns -5 if one is).

Shapes are the smallest each launcher takes (gemm_x3f needs >= 192 workgroups), K = 64 where the split plan
allows.  gemm_x3s never runs TI = 8: it always ties with or loses to TI = 4 and ties go to the smaller tile
(tests/test_trunk_bias_ref_cpu.py shows it on the replica), so TI 4..7 is every height.

Worst observed / allowed ratios are printed per case (run with -s)."""

from __future__ import annotations

import numpy as np
import pytest

import trunk_bias_ref as R

gpu = pytest.mark.gpu

M16, SMALL, BF16, SPLIT, FIN, H2, PONLY = 256, 512, 1024, 2048, 4096, 8192, 32768
PREC_BITS = {"split3": 0, "bf16": BF16, "split2h": H2}


def _up32(v):
    return -(-v // 32) * 32


class Case:
    def __init__(self, name, fam, tile, E, M, N, K, prec, split=False, fin=False, ld_n=None, rows_p=None, k_live=None):
        self.name, self.fam, self.tile = name, fam, tile  # tile: the launch's row tile (gemm_x3s: TI)
        self.E, self.M, self.N, self.K, self.prec, self.split, self.fin, self.k_live = E, M, N, K, prec, split, fin, k_live
        self.ld_n = ld_n if ld_n is not None else _up32(N)       # the engine's padded width
        self.rows_p = rows_p if rows_p is not None else _up32(M + 1)  # at least one padding row
        self.small = fam == 3
        # rows per dbp chunk: the row tile, or the finishing pass's 16 rows
        self.chunk_rows = 16 * tile if self.small else 16 if fam == 2 else tile

    @property
    def bits(self):
        return PREC_BITS[self.prec] | (SMALL if self.small else 0) | (SPLIT if self.split else 0) | (FIN if self.fin else 0)

    @property
    def key(self):
        return (self.E, self.M, self.N, self.K, self.k_live)


def _cases():
    c = []
    for prec in ("split3", "split2h"):  # unsplit, 208-row tiles
        c.append(Case(f"unsplit_ragged_{prec}", 0, 208, 2, 2300, 2040, 64, prec))  # last tile 12 rows, ragged columns
        c.append(Case(f"unsplit_padded_{prec}", 0, 208, 2, 4790, 1000, 64, prec, ld_n=1024, rows_p=4800))
    c.append(Case("bf16_bm400", 0, 400, 2, 6400, 2048, 64, "bf16"))
    c.append(Case("bf16_bm208", 0, 208, 2, 2390, 2040, 64, "bf16"))
    c.append(Case("bf16_bm80", 0, 80, 2, 1280, 2048, 64, "bf16"))
    c.append(Case("bf16_bm48", 0, 48, 2, 1270, 1000, 64, "bf16", ld_n=1024))
    for fin in (False, True):  # split-K: the finishing pass (16-row chunks, M % 16 != 0), the in-launch finish
        f, t = (1, "fin") if fin else (2, "pass")
        c.append(Case(f"split_bm128_{t}", f, 128, 2, 900, 2040, 512, "split3", True, fin))
        c.append(Case(f"split_bm208_{t}", f, 208, 2, 1660, 2040, 512, "split3", True, fin))
        c.append(Case(f"split_3slices_{t}", f, 128, 2, 1270, 1000, 1024, "split3", True, fin, ld_n=1024, k_live=1000))
        c.append(Case(f"split_h2_2slices_{t}", f, 128, 2, 896, 2048, 512, "split2h", True, fin))
    for prec in ("split3", "bf16", "split2h"):  # gemm_x3s at every tile height
        for ti, M in ((4, 100), (5, 260), (6, 330), (7, 390)):
            c.append(Case(f"x3s_ti{ti}_{prec}", 3, ti, 2, M, 2048, 64, prec))
        c.append(Case(f"x3s_w400_padded_{prec}", 3, 5, 2, 1281, 400, 416, prec, ld_n=416, rows_p=1312, k_live=400))
        c.append(Case(f"x3s_one_row_{prec}", 3, 4, 1, 1, 8, 32, prec))
        c.append(Case(f"x3s_tiny_{prec}", 3, 4, 2, 17, 60, 32, prec))
    return c


CASES = _cases()


def test_cases_cover_every_family_and_row_tile():
    """The list as a whole, through the launchers' rules restated in trunk_bias_ref (each GPU case then asserts
    the same through the entry's info): every family, every row tile of each, every precision of gemm_x3s."""
    seen = set()
    for c in CASES:
        if c.small:
            assert R.x3s_ti(c.M, c.N, c.E) == c.tile, c.name
            seen.add(("x3s", c.tile, c.prec))
            continue
        plan = R.x3f_plan(c.M, c.N, -(-c.K // 64) * 64, c.E, c.prec, c.split, c.fin)
        assert plan == (c.fam, c.chunk_rows), (c.name, plan)
        bm, s = R.split_plan(c.M, c.N, -(-c.K // 64) * 64, c.E) if c.split else (c.tile, 1)
        assert bm == c.tile, c.name
        seen.add((R.FAMILIES[c.fam], c.tile, c.prec, s))
    want = {("x3f", 208, "split3", 1), ("x3f", 208, "split2h", 1)}
    want |= {("x3f", bm, "bf16", 1) for bm in (400, 208, 80, 48)}
    for fam in ("x3f_split_fin", "x3f_split_pass"):
        want |= {(fam, 128, "split3", 2), (fam, 208, "split3", 2), (fam, 128, "split3", 3), (fam, 128, "split2h", 2)}
    want |= {("x3s", ti, prec) for ti in (4, 5, 6, 7) for prec in PREC_BITS}
    assert seen >= want, want - seen
    assert any(c.M % 16 for c in CASES if c.fam == 2) and any(c.ld_n > c.N for c in CASES if c.small)


_ref_cache = {}


def _reference(c):
    """Operands and float64 references of a shape, shared by its precisions and forms (the last shape is kept)."""
    k = (c.key, c.prec == "bf16")
    if k not in _ref_cache:
        _ref_cache.clear()
        A, B, bias, mask = R.make_case(c.E, c.M, c.N, c.K, seed=c.M + c.N + c.K, k_live=c.k_live)
        Ar, Br = (R.bf16_rne(A), R.bf16_rne(B)) if c.prec == "bf16" else (A, B)  # bf16: the rounded operands' products
        acc, scale = R.gemm_ref(Ar, Br)
        for a in (A, B, bias, mask, acc, scale):
            a.setflags(write=False)
        _ref_cache[k] = (A, B, bias, mask, acc, scale)
    return _ref_cache[k]


def _run(c, epi, A, B, bias, mask):
    from mtrl_amd import _lib as L

    lib = L.load()
    ponly = bool(epi & PONLY)
    C = None if ponly else np.full((c.E, c.M, c.N), np.nan, np.float32)
    Cs = np.zeros((c.E, c.rows_p, c.ld_n), np.float32)
    maxrt = -(-c.M // 16)
    dbp = np.zeros(c.E * maxrt * c.N, np.float32)
    db = np.zeros((c.E, c.N), np.float32)
    info = np.zeros(8, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    L.check(lib.mtsac_debug_gemm_x3f_ld(epi | c.bits, c.E, c.M, c.N, c.K, c.ld_n, c.rows_p, p(A), p(B), p(C), p(bias),
                                        p(mask), p(Cs), p(dbp), p(db), p(info)))
    assert info[5] == maxrt
    return C, Cs, dbp, db, info


def _ratio(err, tol):
    """max err / tol over the elements (0 / 0 counts as 0); NaN in err fails every bound."""
    assert not np.isnan(err).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def _check(c, epi, label, report):
    A, B, bias, mask, acc, scale = _reference(c)
    ponly = bool(epi & PONLY)
    C, Cs, dbp, db, info = _run(c, epi, A, B, bias if (epi & 255) == 1 else None, mask if (epi & 255) == 2 else None)
    M, N, E, r = c.M, c.N, c.E, c.chunk_rows
    # ---- the form that ran, and the engine's chunk count
    chunks = -(-M // r)
    assert info[0] == c.fam and info[1] == r and info[2] == chunks, (c.name, label, info.tolist())
    assert info[7] == c.tile and (info[3] > 1) == (c.fam in (1, 2)), info.tolist()
    # ---- float64 reference of this epilogue
    if (epi & 255) == 1:
        want = np.maximum(acc + bias[:, None, :], 0)
        etol = R.GEMM_REL * (scale + np.abs(bias[:, None, :])) + 1e-30
        live = np.ones(want.shape, bool)
    else:
        live = mask > 0
        want = np.where(live, acc, 0.0)
        etol = R.GEMM_REL * scale + 1e-30
    # ---- padding untouched, the inside written
    assert np.isnan(Cs[:, M:, :]).all() and np.isnan(Cs[:, :, N:]).all(), (c.name, label, "padding written")
    P = Cs[:, :M, :N].astype(np.float64)
    assert np.isfinite(P).all(), (c.name, label, "plane elements left unwritten")
    # ---- C and the planes inside [M][N]
    if C is not None:
        assert np.isfinite(C).all()
        report[f"{label} C"] = _ratio(np.abs(C - want), etol)
        Cv = C.astype(np.float64)
    else:
        Cv = None
    base = np.abs(want) + etol if Cv is None else np.abs(Cv)  # |C|, or its bound
    if c.prec == "split3":
        ptol = np.zeros_like(want)  # the planes sum back to the fp32 value exactly
    elif c.prec == "bf16":
        ptol = 2.0 ** -8 * base  # the high plane alone
    else:
        ec = int(info[6])
        mB = float(np.abs(B).max())
        if (epi & 255) == 1:
            mB = max(mB, float(np.abs(bias).max()))
        bound = np.float32(c.K) * np.float32(np.abs(A).max()) * np.float32(mB) + (np.float32(mB) if (epi & 255) == 1 else 0)
        assert ec == R.plane_exp(float(bound)), (ec, float(bound))
        ptol = 2.0 ** -21 * base + 1.01 * 2.0 ** (-24 - ec)
    if Cv is not None:
        if c.prec == "split3":
            np.testing.assert_array_equal(Cs[:, :M, :N], C)
        elif c.prec == "bf16":
            np.testing.assert_array_equal(Cs[:, :M, :N], R.bf16_rne(C))
        else:
            report[f"{label} planes-C"] = _ratio(np.abs(P - Cv), ptol)
    report[f"{label} planes"] = _ratio(np.abs(P - want), etol + ptol)
    # ---- dbp: chunks [0, chunks) finite and right, everything after them untouched
    n_live = E * chunks * N
    assert np.isnan(dbp[n_live:]).all(), (c.name, label, "partials past the engine's chunk count were written")
    got = dbp[:n_live].reshape(E, chunks, N).astype(np.float64)
    assert np.isfinite(got).all(), (c.name, label, "a chunk the engine reads was left unwritten")
    rows_in = np.minimum(r, M - r * np.arange(chunks))[None, :, None]
    if Cv is not None:  # against the launch's own fp32 C: any order of r additions
        s, sa = R.chunked_colsum(Cv, r)
        report[f"{label} dbp"] = _ratio(np.abs(got - s), (rows_in - 1) * R.U * sa)
    else:  # against float64: the GEMM bound summed over the chunk's live rows, plus the additions
        s, sa = R.chunked_colsum(want, r)
        st, _ = R.chunked_colsum(np.where(live, etol, 0.0), r)
        report[f"{label} dbp"] = _ratio(np.abs(got - s), st + (rows_in - 1) * R.U * sa)
    # ---- db: colsum_finish over the engine's chunk count
    assert np.isfinite(db).all()
    report[f"{label} db"] = _ratio(np.abs(db - got.sum(axis=1)), R.tol_sum(chunks, np.abs(got).sum(axis=1)))


@gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bias_grad_path(c):
    report = {}
    try:
        _check(c, 2 | M16 | PONLY, "dgrad planes-only", report)
        _check(c, 2 | M16, "dgrad C+planes", report)
        _check(c, 1, "bias+relu", report)
    finally:
        print(f"\n[{c.name}] worst observed / allowed:", {k: round(v, 4) for k, v in report.items()})
    bad = {k: v for k, v in report.items() if not v <= 1.0}
    assert not bad, bad


@gpu
def test_refused_before_any_launch():
    from mtrl_amd import _lib as L

    lib = L.load()
    z = np.zeros(1 << 16, np.float32)
    i8 = np.zeros(8, np.int32)
    P = z.ctypes.data
    run = lambda epi, E, M, N, K, ld, rp: lib.mtsac_debug_gemm_x3f_ld(epi, E, M, N, K, ld, rp, P, P, P, P, P, P, P, P,
                                                                      i8.ctypes.data)
    assert run(1, 1, 16, 64, 64, 32, 16) == -22   # ld_n < N
    assert run(1, 1, 16, 64, 64, 64, 8) == -22    # rows_p < M
    assert run(1, 1, 16, 62, 64, 66, 16) == -22   # ld_n % 4
    assert run(0, 1, 16, 64, 64, 64, 16) == -22   # no store epilogue
    assert run(1, 1, 16, 64, 64, 64, 16) == -95   # gemm_x3f: too few workgroups
    assert run(2 | SMALL, 1, 16, 64, 64, 64, 16) == -95  # gemm_x3s: the mask comes from planes only
    assert lib.mtsac_debug_wgrad_finish(0, 1, 8, 8, 32, 0, 0, P, P, P, None, None, None, P, P, None, None,
                                        i8.ctypes.data) == -22  # no chunks
    assert lib.mtsac_debug_wgrad_finish(1, 1, 8, 8, 32, 1, 0, P, P, P, None, None, None, P, P, None, None,
                                        i8.ctypes.data) == -22  # deferred without the neighbouring jobs


# ------------------------------------------------------------------ the weight grad's finish
WG_SHAPES = [(64, 400, 1280), (39, 400, 96), (256, 128, 6400)]
WG_CHUNKS = [1, 4, 33, 80]  # colsum_final_kernel: the 8-deep loop starts at 29 chunks and steps by 32


def _wgrad(mode, E, M, N, K, chunks, splits, A, B, part, pre=None, post=None):
    from mtrl_amd import _lib as L

    lib = L.load()
    C = np.zeros((E, M, N), np.float32)
    db = np.zeros((E, N), np.float32)
    info = np.zeros(4, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    nb = dpre = dpost = None
    if mode == 1:
        nb = np.array([pre.shape[1], pre.shape[2], post.shape[1], post.shape[2]], np.int32)
        dpre = np.zeros((E, pre.shape[2]), np.float32)
        dpost = np.zeros((E, post.shape[2]), np.float32)
    L.check(lib.mtsac_debug_wgrad_finish(mode, E, M, N, K, chunks, splits, p(A), p(B), p(part), p(nb), p(pre), p(post),
                                         p(C), p(db), p(dpre), p(dpost), p(info)))
    return C, db, dpre, dpost, info


def _db_ratio(db, part):
    p64 = part.astype(np.float64)
    return _ratio(np.abs(db - p64.sum(axis=1)), R.tol_sum(part.shape[1], np.abs(p64).sum(axis=1)))


@gpu
@pytest.mark.parametrize("M,N,K", WG_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in WG_SHAPES])
def test_weight_grad_finishes_the_bias_grad(M, N, K):
    """db from the partials is the same bits whether colsum_finish, the split-K reduce launch or finish_many
    (between two unrelated jobs) adds them, C the same bits at once and deferred, all within the float64 bounds."""
    E = 2
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((E, K, M), dtype=np.float32)
    B = rng.standard_normal((E, K, N), dtype=np.float32)
    acc = A.astype(np.float64).transpose(0, 2, 1) @ B.astype(np.float64)
    scale = np.abs(A.astype(np.float64)).transpose(0, 2, 1) @ np.abs(B.astype(np.float64))
    pre = rng.standard_normal((E, 37, 72), dtype=np.float32)
    post = rng.standard_normal((E, 5, 130), dtype=np.float32)
    report = {}
    for chunks in WG_CHUNKS:
        part = rng.standard_normal((E, chunks, N), dtype=np.float32)
        C1, db1, _, _, i1 = _wgrad(0, E, M, N, K, chunks, 1, A, B, part)  # no split: colsum_finish
        assert i1[0] == 1 and i1[1] == 0, i1.tolist()
        C0, db0, _, _, i0 = _wgrad(0, E, M, N, K, chunks, 0 if K >= 1280 else 2, A, B, part)  # the reduce launch
        assert i0[0] > 1 and i0[1] == 1, i0.tolist()
        Cd, dbd, dpre, dpost, idf = _wgrad(1, E, M, N, K, chunks, 0 if K >= 1280 else 2, A, B, part, pre, post)
        assert idf[0] == i0[0] and idf[1] == 2 and idf[2] == 3 and idf[3] > 0, idf.tolist()
        np.testing.assert_array_equal(db0, db1)
        np.testing.assert_array_equal(dbd, db1)
        np.testing.assert_array_equal(Cd, C0)
        # deferred without split-K: the sink holds a plain colsum job for it
        Ce, dbe, epre, epost, ie = _wgrad(1, E, M, N, K, chunks, 1, A, B, part, pre, post)
        assert ie[0] == 1 and ie[1] == 2 and ie[2] == 3 and ie[3] == 0, ie.tolist()
        np.testing.assert_array_equal(dbe, db1)
        np.testing.assert_array_equal(Ce, C1)
        np.testing.assert_array_equal(epre, dpre)
        np.testing.assert_array_equal(epost, dpost)
        report[f"chunks {chunks} db"] = _db_ratio(db1, part)
        report[f"chunks {chunks} C"] = max(_ratio(np.abs(C - acc), R.GEMM_REL * scale + 1e-30) for C in (C1, C0))
        report[f"chunks {chunks} neighbours"] = max(_db_ratio(dpre, pre), _db_ratio(dpost, post))
    print(f"\n[wgrad {M}x{N}x{K}] slices {int(i0[0])}, worst observed / allowed:",
          {k: round(v, 4) for k, v in report.items()})
    bad = {k: v for k, v in report.items() if not v <= 1.0}
    assert not bad, bad
