"""The layout kernels on their own (mtsac_debug_layout): split_planes in its row form, its 64 x 64 LDS tile
form and transposed, in the fragment layout, split3 and split2h, batch 2; transpose_f32; colsum in its vector
and scalar forms.  The planes are compared word for word with tests/trunk_bias_ref.py, the outputs are guarded
and start as all-ones words, so both a missing zero fill and a write outside [out_rows][out_cols] show.

Zero fill: the row form writes all of [out_rows][out_cols].  The tile form's grid covers the source's 64 x 64
tiles only, so output past them is left alone.  The engine never relies on a fill there: its only tile-form
launches are the transposed weight planes, whose out_cols (the padded in-dim, a multiple of 32 or 64 no larger
than the source rows rounded up to 64) and out_rows (= the source columns) lie inside the source's tiles, and
every plane buffer is allocated zeroed.  So the tests assert that region stays untouched.

Every kernel is run twice and must give the same bits."""

from __future__ import annotations

import numpy as np
import pytest

import trunk_bias_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from mtrl_amd import _lib as L

    return L, L.load()


def _split(x, ldx, out_rows, out_cols, ldo, arows, tr=False, frag=False, e2h=None):
    """x [batch][rows][cols] laid out with row stride ldx -> the plane words [batch][3][arows * ldo], run twice."""
    L, lib = _lib()
    batch, rows, cols = x.shape
    src = np.full((batch, rows, ldx), 7.25, np.float32)  # the source's own padding must never be read into a plane
    src[:, :, :cols] = x
    dims = np.array([rows, cols, ldx, out_rows, out_cols, ldo, arows, int(tr), batch, int(frag), int(e2h is not None),
                     e2h or 0], np.int32)
    outs = []
    for _ in range(2):
        out = np.zeros((batch, 3, arows * ldo), np.uint16)
        L.check(lib.mtsac_debug_layout(0, dims.ctypes.data, src.ctypes.data, out.ctypes.data, None))
        outs.append(out)
    np.testing.assert_array_equal(outs[0], outs[1])
    return outs[0]


def _values(rows, cols, e2h, seed):
    rng = np.random.default_rng(seed)
    top = np.float32(2.0 ** (15 - (e2h or 0)))
    x = rng.standard_normal((2, rows, cols), dtype=np.float32) * (top / np.float32(8) if e2h is not None else np.float32(3))
    x = np.clip(x, -top * np.float32(0.999), top * np.float32(0.999))
    special = np.array([0.0, -0.0, 1e-30, -1e-30, top * np.float32(1 - 2.0 ** -12), -top * np.float32(1 - 2.0 ** -12),
                        top * np.float32(2.0 ** -26), 1.0], np.float32)
    if e2h is not None:
        # -0.0 is left out of the fp16 cases: its planes are a zero of either sign (the device writes h = +0,
        # l = -0, numpy's conversions h = -0, l = +0), the same value and the same mask bit
        special[1] = 0.5
    flat = x.reshape(2, -1)
    n = min(flat.shape[1], special.size)
    flat[:, :n] = special[:n]
    return x


def _pad4(v):
    return -(-v // 4) * 4


def _off4(v):  # the next size that is no multiple of 4
    return v + 1 if (v + 1) % 4 else v + 2


SHAPES = [(1, 1), (63, 65), (64, 64), (130, 39), (400, 416)]


@pytest.mark.parametrize("rows,cols", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
@pytest.mark.parametrize("form", ["rows", "rows_scalar_loads", "tiles", "transposed"])
def test_split_planes_split3(rows, cols, form):
    x = _values(rows, cols, None, rows + cols)
    tr = form == "transposed"
    ldx = _off4(cols) if form == "rows_scalar_loads" else _pad4(cols) + (4 if form == "rows" else 0)
    if tr:  # out_rows past the source columns, out_cols past the next multiple of 64 of the source rows
        out_rows, out_cols = cols + 5, -(-rows // 64) * 64 + 70
    elif form == "tiles":  # out_cols no multiple of 4: the LDS tile form
        out_rows, out_cols = rows + 70, _off4(cols + 64)
    else:
        out_rows, out_cols = rows + 37, _pad4(cols) + 32
    ldo, arows = _pad4(out_cols) + 8, out_rows + 3
    got = _split(x, ldx, out_rows, out_cols, ldo, arows, tr=tr)
    want = R.split_planes(x, out_rows, out_cols, ldo, arows, transpose=tr)
    np.testing.assert_array_equal(got, want)
    assert (want == R.UNTOUCHED).any() and (want[:, :, :1] != R.UNTOUCHED).all()


@pytest.mark.parametrize("rows,cols", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
@pytest.mark.parametrize("tr", [False, True], ids=["rows", "transposed"])
@pytest.mark.parametrize("e2h", [None, 0], ids=["split3", "split2h"])
def test_split_planes_fragment_layout(rows, cols, tr, e2h):
    x = _values(rows, cols, e2h, 3 * rows + cols)
    srows, scols = (cols, rows) if tr else (rows, cols)
    out_rows, out_cols = -(-srows // 16) * 16, -(-scols // 32) * 32
    ldo, arows = out_cols + 32, out_rows + 16
    got = _split(x, _pad4(cols), out_rows, out_cols, ldo, arows, tr=tr, frag=True, e2h=e2h)
    want = R.split_planes(x, out_rows, out_cols, ldo, arows, transpose=tr, frag=True, e2h=e2h)
    np.testing.assert_array_equal(got, want)
    on = R.split_planes(x, out_rows, out_cols, ldo, arows, transpose=tr, frag=False, e2h=e2h)
    assert rows * cols < 64 or not np.array_equal(on, want)  # the layout does move elements


@pytest.mark.parametrize("e", [-20, 0, 14])
@pytest.mark.parametrize("rows,cols,tr", [(63, 65, False), (63, 65, True), (400, 416, False), (130, 39, True)],
                         ids=["63x65", "63x65_t", "400x416", "130x39_t"])
def test_split_planes_split2h(e, rows, cols, tr):
    """Two fp16 planes of x 2^e: zero, -0, +-1e-30 (the sticky subnormal keeps the positive one visible), values just
    under 2^(15 - e); the third plane is never written."""
    x = _values(rows, cols, e, rows + cols + 20 + e)
    srows, scols = (cols, rows) if tr else (rows, cols)
    out_rows, out_cols = srows + 9, _pad4(scols) + 12
    ldo, arows = out_cols + 4, out_rows + 2
    got = _split(x, _pad4(cols), out_rows, out_cols, ldo, arows, tr=tr, e2h=e)
    want = R.split_planes(x, out_rows, out_cols, ldo, arows, transpose=tr, e2h=e)
    np.testing.assert_array_equal(got, want)
    assert (got[:, 2] == R.UNTOUCHED).all()
    w = got.reshape(2, 3, arows, ldo)
    src = x.transpose(0, 2, 1) if tr else x
    pos = R.split2h_positive(w[:, 0, :srows, :scols], w[:, 1, :srows, :scols])
    nn = ~np.signbit(src)
    assert np.array_equal(pos[nn], src[nn] > 0)


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (130, 39), (257, 64)],
                         ids=lambda v: str(v))
def test_transpose_f32(rows, cols):
    L, lib = _lib()
    x = np.random.default_rng(rows * cols).standard_normal((2, rows, cols), dtype=np.float32)
    dims = np.array([rows, cols, 2], np.int32)
    outs = []
    for _ in range(2):
        out = np.zeros((2, cols, rows), np.float32)
        L.check(lib.mtsac_debug_layout(1, dims.ctypes.data, x.ctypes.data, out.ctypes.data, None))
        outs.append(out)
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    np.testing.assert_array_equal(outs[0].view(np.uint32), np.ascontiguousarray(x.transpose(0, 2, 1)).view(np.uint32))


@pytest.mark.parametrize("cols", [4, 100, 401, 2048])
@pytest.mark.parametrize("rows", [1, 3, 255, 257, 1000, 20000])
def test_colsum(rows, cols):
    """db and the per-chunk partials within (n - 1) U sum|x| of float64 (n values added in some order); 401
    columns take the scalar kernel.  chunks = min(64, ceil(rows / 256)) of ceil(rows / chunks) rows each; the
    partial buffer past them stays NaN."""
    L, lib = _lib()
    batch = 2 if rows * cols < 4_000_000 else 1
    ld = cols + 4 if cols % 4 == 0 else cols
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((batch, rows, ld), dtype=np.float32)
    dims = np.array([rows, cols, ld, batch], np.int32)
    outs = []
    for _ in range(2):
        part = np.zeros(batch * 64 * cols, np.float32)
        db = np.zeros((batch, cols), np.float32)
        L.check(lib.mtsac_debug_layout(2, dims.ctypes.data, x.ctypes.data, part.ctypes.data, db.ctypes.data))
        outs.append((part, db))
    np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    np.testing.assert_array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    part, db = outs[0]
    x64 = x[:, :, :cols].astype(np.float64)
    chunks = max(1, min(64, -(-rows // 256)))
    per = -(-rows // chunks)
    n_live = batch * chunks * cols
    assert np.isnan(part[n_live:]).all()
    got = part[:n_live].reshape(batch, chunks, cols).astype(np.float64)
    s, sa = R.chunked_colsum(x64, per)
    assert s.shape[1] == chunks
    rows_in = np.minimum(per, rows - per * np.arange(chunks))[None, :, None]
    worst_part = np.abs(got - s) - (rows_in - 1) * R.U * sa
    assert not np.isnan(got).any() and (worst_part <= 0).all(), float(worst_part.max())
    err, tol = np.abs(db - x64.sum(axis=1)), R.tol_sum(rows, np.abs(x64).sum(axis=1))
    assert not np.isnan(db).any() and (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    print(f"\n[colsum {rows}x{cols}] worst db err / allowed:", float((err / np.maximum(tol, 1e-300)).max()) if rows > 1 else 0.0)
