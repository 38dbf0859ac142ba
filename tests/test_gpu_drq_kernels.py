"""The DrQ kernels of mtrl_amd/csrc/drq.hip one by one (the single-kernel entry points of
include/mtsac_debug.h) against the plain float64 references of tests/drq_kernel_ref.py, at edge
shapes, every channel pair and flag combination, and every conv family forced through the debug
masks -- with the family asserted through mtsac_debug_drq_conv_path before each launch.

Every device output starts as NaN between two guard bands: an element a kernel leaves alone fails the
no-NaN assertion, a store outside the buffer fails the call (-5).

Bars (err against the float64 reference, S = the sum of the |terms| of the output):
 * fp32 forward / data grad: (9 KI + 2) 2^-24 S, KI the summed channel count -- the worst-case
   rounding of an fmaf chain of that length in any order (bias / residual / mask included).  A wrong
   tap is off by O(S).
 * weight / bias grads: 2e-6 S, the bar test_gemm_store holds fp32 sums to.
 * split2h: the smaller of that + 2^-20 S (two operand splits and the dropped l l product, 2^-22
   each, one spare) and 4e-6 S (the project's bar for split precision), plus the absolute floor
   H2_FLOOR 9 KI max|x| max|w| derived at H2_FLOOR below.
Each test prints its worst err / bound (recorded in profiles/drq_kernel_tests.txt)."""

from __future__ import annotations

import contextlib
import functools

import numpy as np
import pytest

import drq_kernel_ref as R

pytestmark = pytest.mark.gpu

PAIRS = [(4, 8), (8, 8), (8, 16), (16, 16)]
SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 2, 2), (2, 3, 7), (2, 7, 3), (2, 11, 11), (2, 21, 21), (2, 16, 15),
          (2, 15, 16), (1, 20, 32), (1, 20, 33), (1, 23, 40), (1, 43, 84), (1, 2, 300)]
EPS = 2.0 ** -24
WGRAD_TOL = 2e-6
SPLIT_REL = 4e-6
# The split2h kernel scales a tile by 2^e, e from the tile's max |x|: bound = 1.00390625 max|x| and
# bound 2^e in [2^14, 2^15), so 2^-e <= 1.00390625 max|x| 2^-14.  A scaled value y is kept as
# h = fp16(y), l = fp16(y - h); the low plane bottoms out at the fp16 subnormal spacing 2^-24, so
# |y - h - l| <= 2^-25 in scaled units wherever the relative 2^-22 |y| is smaller: an absolute
# |dx| <= 2^-25 2^-e <= 1.00390625 2^-39 max|x|, and likewise |dw| for the weights (one exponent for
# all of them).  An output sums 9 KI products, each off by at most |dx| |w| + |x| |dw|
# <= 2 x 1.00390625 2^-39 max|x| max|w|; the cross terms with the dropped l l product at the floor
# are 2^-12 of that (the 1 + 2^-11).
H2_FLOOR = 2 * 1.00390625 * (1 + 2.0 ** -11) * 2.0 ** -39


def _lib():
    from mtrl_amd import _lib as L

    return L.load()


@contextlib.contextmanager
def _masks(legacy=0, groups=(0, 0), wg_blocks=0):
    lib = _lib()
    old = (lib.mtsac_debug_drq_legacy(-1), lib.mtsac_debug_drq_wgrad_blocks(-1))
    old_g = lib.mtsac_debug_drq_groups(*groups)
    try:
        lib.mtsac_debug_drq_legacy(legacy)
        lib.mtsac_debug_drq_wgrad_blocks(wg_blocks)
        yield
    finally:
        lib.mtsac_debug_drq_legacy(old[0])
        lib.mtsac_debug_drq_wgrad_blocks(old[1])
        lib.mtsac_debug_drq_groups(old_g & 255, old_g >> 8)


@functools.lru_cache(maxsize=None)
def _ops(shape, pair):
    """The operands of one (shape, channel pair), float32, drawn once."""
    B, H, W = shape
    ci, co = pair
    rng = np.random.default_rng(1000 * B + 100 * H + W + 7 * ci + co)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    o = dict(x=f(B, H, W, ci), w=f(3, 3, ci, co), bias=f(co), res=f(B, H, W, co), dout=f(B, H, W, co),
             mask=f(B, H, W, ci), dres=f(B, H, W, ci), w2=f(3, 3, ci, co), bias2=f(co))
    o["mask"].flat[::3] = 0.0  # the mask is strictly > 0: zeros of either sign block the gradient
    o["mask"].flat[1::5] = -0.0
    for v in o.values():
        v.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, pair, flags):
    """(reference, S) of one case, computed once and shared by the families."""
    o = _ops(shape, pair)
    if kind == 0:
        relu, res = flags
        return R.conv_fwd(o["x"], o["w"], o["bias"], relu, o["res"] if res else None)
    if kind == 1:
        mask, dres = flags
        return R.conv_bwd_data(o["dout"], o["w"], o["mask"] if mask else None, o["dres"] if dres else None)
    return R.conv_wgrad(o["x"], o["dout"], flags[0])


def _path(kind, shape, pair):
    from mtrl_amd.drq import debug_conv_path

    return debug_conv_path(kind, *shape, *pair)


def _tiled_fits(kind, family, shape, pair):
    """Whether the tiled family takes the shape: the forward / data-grad row tiles stage three
    padded rows of the summed channels in 4096 floats of LDS and hold at most 256 pixels a tile, the
    split2h planes hold 6144 fp16 a plane; the row-tile weight grad takes every width up to 84
    (and a 300-wide row at 4 input channels); nothing tiled takes W < 2."""
    W = shape[2]
    ki = pair[0] if kind == 0 else pair[1]
    if W < 2:
        return False
    if kind == 2:
        return W <= 84 or pair[0] == 4
    return 3 * (W + 2) * ki <= (4096 if family == 1 else 6144) and (family == 2 or W <= 256)


def _run(kind, shape, pair, flags, defer=False):
    from mtrl_amd import drq as D

    o = _ops(shape, pair)
    if kind == 0:
        return D.debug_conv_fwd(o["x"], o["w"], o["bias"], flags[0], o["res"] if flags[1] else None)
    if kind == 1:
        return D.debug_conv_bwd_data(o["dout"], o["w"], o["mask"] if flags[0] else None, o["dres"] if flags[1] else None)
    return D.debug_conv_wgrad(o["x"], o["dout"], flags[0], defer)


def _bound(kind, family, shape, pair, flags, S):
    ki = pair[0] if kind == 0 else pair[1]
    rel = (9 * ki + 2) * EPS
    if family != 2:
        return rel * S
    o = _ops(shape, pair)
    x = o["x"] if kind == 0 else o["dout"]
    if kind == 0 and flags[0]:
        x = np.maximum(x, 0)
    mx = np.abs(x).reshape(shape[0], -1).max(1).reshape(-1, 1, 1, 1).astype(np.float64)  # per image >= per tile
    return min(rel + 2.0 ** -20, SPLIT_REL) * S + H2_FLOOR * 9 * ki * mx * float(np.abs(o["w"]).max())


FLAGS = {0: [(r, s) for r in (False, True) for s in (False, True)],
         1: [(m, d) for m in (False, True) for d in (False, True)],
         2: [(False,), (True,)]}
# family -> {kind: masks}: the existing switches that force it
FORCE = {
    "pixel": (0, {0: dict(legacy=1 | 16), 1: dict(legacy=2 | 16), 2: dict(legacy=4 | 16)}),
    "pixel_g4": (0, {0: dict(legacy=1 | 16, groups=(4, 4)), 1: dict(legacy=2 | 16, groups=(4, 4))}),
    "pixel_g8": (0, {0: dict(legacy=1 | 16, groups=(8, 8)), 1: dict(legacy=2 | 16, groups=(8, 8))}),
    "rows": (1, {0: dict(legacy=16), 1: dict(legacy=16 | 8), 2: dict(legacy=16 | 8)}),
    "split2h": (2, {0: dict(legacy=32), 1: dict(legacy=32)}),
}
CASES = [(k, f) for f, (_, by_kind) in FORCE.items() for k in by_kind]


@pytest.mark.parametrize("kind,force", CASES, ids=[f"{('fwd', 'bwd_data', 'wgrad')[k]}-{f}" for k, f in CASES])
def test_conv_family(kind, force):
    """One conv direction on one kernel family, every shape x channel pair x flag combination."""
    family, by_kind = FORCE[force]
    worst, worst_case, short_tile, ran = 0.0, None, False, 0
    # the row-tile weight grad shortens its tiles only once the batch gives 512 of them: one wide
    # batch of tiny images for its short last tile
    shapes = SHAPES + ([(256, 3, 7)] if kind == 2 else [])
    with _masks(**by_kind[kind]):
        for shape in shapes:
            for pair in PAIRS:
                if family == 2 and kind == 0 and pair[0] < 8:
                    continue  # the split2h forward takes 8 and 16 input channels
                want = family if family in (0, 3) or _tiled_fits(kind, family, shape, pair) else 0
                fam, rows, tiles, blocks = _path(kind, shape, pair)
                assert fam == want, (force, kind, shape, pair, (fam, rows, tiles, blocks))
                if shape[2] < 2 or (shape[2] == 300 and not (kind == 2 and pair[0] == 4)):
                    assert fam in (0, 3), (shape, pair, fam)  # every tiled family falls back
                if fam in (1, 2):
                    assert rows >= 1 and tiles * rows >= shape[1] and blocks >= 1, (shape, pair, rows, tiles)
                    short_tile |= tiles * rows > shape[1]
                for flags in FLAGS[kind]:
                    case = (force, kind, shape, pair, flags)
                    got = _run(kind, shape, pair, flags)
                    ref = _ref(kind, shape, pair, flags)
                    if kind == 2:
                        pairs_ = [(got[0], ref[0], WGRAD_TOL * ref[2]), (got[1], ref[1], WGRAD_TOL * ref[3])]
                    else:
                        pairs_ = [(got, ref[0], _bound(kind, fam, shape, pair, flags, ref[1]))]
                    for g, r, bound in pairs_:
                        assert not np.isnan(g).any(), ("unwritten output", case)
                        err = np.abs(g.astype(np.float64) - r)
                        ratio = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
                        assert (err <= bound).all(), (case, "worst err / bound", ratio, "at",
                                                      np.unravel_index(np.argmax(err - bound), err.shape))
                        if ratio > worst:
                            worst, worst_case = ratio, case
                    ran += 1
    if family in (1, 2):
        assert short_tile, "no case with a short last tile (n R > H)"
    print(f"drq conv {('forward', 'data grad', 'weight grad')[kind]} {force}: {ran} cases, worst err / bound "
          f"{worst:.3f} at {worst_case}")


def test_default_selection_flips_where_documented():
    """Default masks: rows versus pixel at W = 15 | 16, split2h versus not at W = 32 | 33 with 16
    summed channels."""
    with _masks():
        for pair in PAIRS:
            ci, co = pair
            # weight grad: row tiles from W = 16, im2col below
            assert _path(2, (2, 16, 15), pair)[0] == 0 and _path(2, (2, 15, 16), pair)[0] == 1, pair
            # forward: split2h for 16 input channels at W <= 32, row tiles otherwise
            assert _path(0, (1, 20, 32), pair)[0] == (2 if ci == 16 else 1), pair
            assert _path(0, (1, 20, 33), pair)[0] == 1, pair
            # data grad (summed channels = co): split2h at W <= 32, row tiles above; 8 channels: pixel
            assert _path(1, (1, 20, 32), pair)[0] == (2 if co == 16 else 0), pair
            assert _path(1, (1, 20, 33), pair)[0] == (1 if co == 16 else 0), pair
    with _masks(legacy=16):  # without split2h the data grad's own cut-off shows: rows for co = 16, W >= 16
        for pair in PAIRS:
            assert _path(1, (2, 16, 15), pair)[0] == 0, pair
            assert _path(1, (2, 15, 16), pair)[0] == (1 if pair[1] == 16 else 0), pair


@pytest.mark.parametrize("force", ["pixel", "rows", "split2h", "default"])
def test_conv_forward_two_parameter_sets(force):
    """Images [B1, B) on the second parameter set, B1 = 0..B; B1 H W a multiple of 256 and not."""
    from mtrl_amd.drq import debug_conv_fwd

    family, masks = (None, {}) if force == "default" else (FORCE[force][0], FORCE[force][1][0])
    worst, B = 0.0, 3
    with _masks(**masks):
        for H, W in ((11, 11), (16, 16)):
            for pair in PAIRS:
                if family == 2 and pair[0] < 8:
                    continue
                shape = (B, H, W)
                fam = _path(0, shape, pair)[0]
                assert family is None or fam == family, (force, shape, pair, fam)
                o = _ops(shape, pair)
                for B1 in range(B + 1):
                    got = debug_conv_fwd(o["x"], o["w"], o["bias"], True, o["res"], o["w2"], o["bias2"], B1)
                    ref, S = R.conv_fwd(o["x"], o["w"], o["bias"], True, o["res"], o["w2"], o["bias2"], B1)
                    assert not np.isnan(got).any(), (force, shape, pair, B1)
                    bound = _bound(0, fam, shape, pair, (True, True), S)
                    if fam == 2:  # the floor takes the larger of the two weight sets
                        bound = bound + H2_FLOOR * 9 * pair[0] * float(np.abs(o["x"]).max() * np.abs(o["w2"]).max())
                    err = np.abs(got - ref)
                    assert (err <= bound).all(), (force, shape, pair, B1, float((err / bound).max()))
                    worst = max(worst, float((err / bound).max()))
    print(f"drq conv forward two parameter sets {force}: worst err / bound {worst:.3f}")


def test_conv_wgrad_grid_cap():
    """The row-tile weight grad below and above its grid cap (several tiles a block; more blocks
    asked for than tiles), reduced directly and through the update's deferred segment sum."""
    worst = 0.0
    for cap in (3, 100000):
        with _masks(legacy=16 | 8, wg_blocks=cap):
            for shape in ((2, 11, 11), (2, 21, 21), (1, 23, 40), (3, 2, 2)):
                for pair in PAIRS:
                    fam, rows, tiles, blocks = _path(2, shape, pair)
                    assert fam == 1 and blocks == min(cap, shape[0] * tiles), (cap, shape, pair, rows, tiles, blocks)
                    for relu in (False, True):
                        dw_r, db_r, Sw, Sb = _ref(2, shape, pair, (relu,))
                        for defer in (False, True):
                            dw, db = _run(2, shape, pair, (relu,), defer)
                            assert not np.isnan(dw).any() and not np.isnan(db).any(), (cap, shape, pair, relu, defer)
                            for g, r, S in ((dw, dw_r, Sw), (db, db_r, Sb)):
                                err = np.abs(g - r)
                                assert (err <= WGRAD_TOL * S).all(), (cap, shape, pair, relu, defer,
                                                                      float((err / (WGRAD_TOL * S)).max()))
                                worst = max(worst, float((err / np.maximum(WGRAD_TOL * S, 1e-300)).max()))
    print(f"drq conv weight grad grid cap: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("kind", [0, 1], ids=["fwd", "bwd_data"])
def test_split2h_dynamic_range_floor(kind):
    """One pixel at 1e4 beside 1e-3 everywhere else, in one tile: the tile's exponent comes from the
    1e4, so the small entries sit on the low plane's absolute floor.  The kernel is held to exactly
    the floor derived at H2_FLOOR (no relative slack beyond the split2h bar)."""
    from mtrl_amd import drq as D

    worst = 0.0
    with _masks(legacy=32):
        for pair in [(8, 8), (8, 16), (16, 16)] if kind == 0 else PAIRS:
            ci, co = pair
            shape = (1, 8, 8)
            fam, rows, tiles, _ = _path(kind, shape, pair)
            assert (fam, tiles) == (2, 1) and rows == 8, (pair, fam, rows, tiles)  # one tile: one exponent
            ki = ci if kind == 0 else co
            rng = np.random.default_rng(77 + ci + co)
            x = (1e-3 * rng.choice([-1.0, 1.0], (1, 8, 8, ki))).astype(np.float32)
            x[0, 3, 4, :] = 1e4
            w = rng.standard_normal((3, 3, ci, co)).astype(np.float32)
            if kind == 0:
                got = D.debug_conv_fwd(x, w, np.zeros(co, np.float32))
                ref, S = R.conv_fwd(x, w, np.zeros(co))
            else:
                got = D.debug_conv_bwd_data(x, w)
                ref, S = R.conv_bwd_data(x, w)
            assert not np.isnan(got).any(), pair
            bound = SPLIT_REL * S + H2_FLOOR * 9 * ki * float(np.abs(x).max()) * float(np.abs(w).max())
            err = np.abs(got - ref)
            far = np.ones((8, 8), bool)
            far[2:5, 3:6] = False  # outputs that do not see the large pixel: the floor is all they have
            ratio, ratio_far = float((err / bound).max()), float((err[0][far] / bound[0][far]).max())
            assert (err <= bound).all(), (pair, ratio, ratio_far)
            worst = max(worst, ratio)
            print(f"drq conv split2h dynamic range {('forward', 'data grad')[kind]} {pair}: err / bound {ratio:.3f} "
                  f"(away from the large pixel {ratio_far:.3f}, floor / S there "
                  f"{float((bound[0][far] / S[0][far]).max() - SPLIT_REL):.2e})")
    assert worst > 0


def test_debug_entries_refuse_bad_arguments():
    """-22 before anything is launched: sizes, an uninstantiated channel pair, a short ldh."""
    from mtrl_amd import _lib as L
    from mtrl_amd import drq as D

    f = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_conv_fwd(f(1, 4, 4, 4), f(3, 3, 4, 4), f(4))  # 4 -> 4 is not instantiated
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_conv_path(3, 1, 4, 4, 4, 8)
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_conv_path(0, 0, 4, 4, 4, 8)
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_conv_fwd(f(2, 4, 4, 4), f(3, 3, 4, 8), f(8), w2=f(3, 3, 4, 8), bias2=f(8), B1=3)
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_maxpool(f(1, 4, 4, 6), f(1, 2, 2, 6))
    A, Z = 2, 65
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_c51(f(1, 3 * Z), f(1, 3 * Z), f(1, 3 * Z), f(3 * Z), f(3 * Z), f(1), f(1), [0], A, Z, 0.97, -10.0, 10.0)
    Z = 8
    with pytest.raises(L.MTSACError, match="-22"):
        D.debug_c51(f(1, 3 * Z - 1), f(1, 3 * Z - 1), f(1, 3 * Z - 1), f(3 * Z), f(3 * Z), f(1), f(1), [0], A, Z, 0.97,
                    -10.0, 10.0)


# ---------------------------------------------------------------- max pool
POOL_SHAPES = [(1, 1), (1, 4), (2, 2), (3, 3), (4, 5), (5, 4), (7, 7), (10, 10), (21, 21), (20, 11)]


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_maxpool_equals_reference(kind):
    """out, argmax tap and din equal the reference: SAME padding per axis (4 x 5 pads no row and
    one column), the first maximum in row-major order on ties (values from {0, 1, 2}: ties
    everywhere), dout small integers so that din is exact."""
    from mtrl_amd.drq import debug_maxpool

    n = 0
    for C in (8, 16):
        for H, W in POOL_SHAPES:
            for B in (1, 3):
                rng = np.random.default_rng(100 * H + W + C + B)
                shape = (B, H, W, C)
                x = (rng.standard_normal(shape) if kind == "normal" else rng.integers(0, 3, shape)).astype(np.float32)
                dout = rng.integers(-4, 5, (B, (H + 1) // 2, (W + 1) // 2, C)).astype(np.float32)
                out, arg, din = debug_maxpool(x, dout)
                r_out, r_arg, r_din = R.maxpool(x, dout)
                case = (kind, C, H, W, B)
                assert not np.isnan(out).any() and not np.isnan(din).any() and (arg < 9).all(), case
                np.testing.assert_array_equal(out, r_out, err_msg=str(case))
                np.testing.assert_array_equal(arg, r_arg, err_msg=str(case))
                np.testing.assert_array_equal(din, r_din, err_msg=str(case))
                n += 1
    print(f"drq max pool {kind}: {n} cases equal")


# ---------------------------------------------------------------- dueling head + C51
C51_CONFIGS = [(18, 51), (1, 2), (7, 64), (6, 40), (5, 59), (3, 33)]
GAMMA, NSTEP, VMIN, VMAX = 0.99, 3, -10.0, 10.0
ROW_KINDS = ("generic", "clamped_high", "clamped_low", "done_zero", "done_support", "done_vmax")


def _c51_rows(kinds, Z, rng):
    sup = R.c51_index_f32([0.0], [0.0], Z, GAMMA, NSTEP, VMIN, VMAX)[0]
    rew = {"generic": None, "clamped_high": 25.0, "clamped_low": -25.0, "done_zero": 0.0,
           "done_support": float(sup[Z // 3]), "done_vmax": VMAX}
    r = np.array([np.round(rng.standard_normal() * 2, 3) if rew[k] is None else rew[k] for k in kinds], np.float32)
    d = np.array([1.0 if k.startswith("done") else 0.0 for k in kinds], np.float32)
    return r, d


def _c51_case(A, Z, ldh, kinds, seed0):
    """Operands whose two best reference q differ by >= 1e-3 in every row (so that a_next is not
    decided by rounding): the first seed from seed0 on that has the gap; returns the reference too."""
    B = len(kinds)
    for seed in range(seed0, seed0 + 20):
        rng = np.random.default_rng(seed)
        hs, hn, ht = ((3 * rng.standard_normal((B, ldh))).astype(np.float32) for _ in range(3))
        bo, bt = (rng.standard_normal((A + 1) * Z).astype(np.float32) for _ in range(2))
        rew, done = _c51_rows(kinds, Z, rng)
        act = rng.integers(0, A, B).astype(np.int32)
        ref = R.c51(hs, hn, ht, bo, bt, rew, done, act, A, Z, GAMMA, NSTEP, VMIN, VMAX)
        q = np.sort(ref[2], -1)
        if A == 1 or (q[:, -1] - q[:, -2]).min() >= 1e-3:
            return (hs, hn, ht, bo, bt, rew, done, act), ref
    raise AssertionError(("no seed with a q gap", A, Z, kinds))


def test_c51_trio_matches_reference():
    """c51_target, q_values and c51_loss at atom counts 2..64 (every lane busy at 64), padded and
    dense head rows, one and five rows; rows that sit on the projection's discontinuity (clamped
    high / low, episode ends with the reward on a support point) are exact in float32 whether or not
    the compiler contracts rew + g (1 - done) sup, and the reference decides them in float32 too."""
    from mtrl_amd.drq import debug_c51

    gn = float(np.float32(GAMMA ** NSTEP))
    worst, n, dropped = {}, 0, 0
    for A, Z in C51_CONFIGS:
        for ldh in ((A + 1) * Z, (A + 1) * Z + 3):
            batches = [(k,) for k in ROW_KINDS] + [tuple(ROW_KINDS[(s + i) % 6] for i in range(5)) for s in (0, 3)]
            for bi, kinds in enumerate(batches):
                B = len(kinds)
                ops, ref = _c51_case(A, Z, ldh, kinds, 1000 * A + 10 * Z + bi)
                m_r, an_r, q_r, dh_r, lb_r, gb_r = ref
                if A > 1:
                    qs = np.sort(q_r, -1)
                    assert (qs[:, -1] - qs[:, -2]).min() >= 1e-3
                m, an, q, dh, lb, gb = debug_c51(*ops, A, Z, gn, VMIN, VMAX)
                case = (A, Z, ldh, kinds)
                used = (A + 1) * Z
                for name, v in (("m", m), ("q", q), ("dh", dh[:, :used]), ("loss_b", lb), ("logit_b", gb)):
                    assert not np.isnan(v).any(), (name, case)
                assert np.isnan(dh[:, used:]).all(), ("dh written past (A + 1) Z", case)
                np.testing.assert_array_equal(an, an_r, err_msg=str(case))
                for b in range(B):  # a row whose whole mass is dropped is exactly zero on the device too
                    if (m_r[b] == 0).all():
                        assert (m[b] == 0).all(), ("dropped mass", case, b, m[b].sum())
                        dropped += 1
                    elif kinds[b] != "generic":  # all of it kept, on one or two atoms
                        assert abs(float(m[b].astype(np.float64).sum()) - 1.0) <= 1e-5, (case, b, m[b].sum())
                for name, g, r in (("m", m, m_r), ("q", q, q_r), ("loss_b", lb, lb_r), ("logit_b", gb, gb_r)):
                    ratio = float((np.abs(g - r) / (1e-5 * np.maximum(1.0, np.abs(r)))).max())
                    worst[name] = max(worst.get(name, 0.0), ratio)
                    assert ratio <= 1.0, (name, case, ratio)
                ratio = float(np.abs(dh[:, :used] - dh_r[:, :used]).max() / (1e-5 / B))
                worst["dh"] = max(worst.get("dh", 0.0), ratio)
                assert ratio <= 1.0, ("dh", case, ratio)
                n += 1
    assert dropped > 0
    print(f"drq c51 trio: {n} cases ({dropped} rows with all mass dropped), worst err / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
