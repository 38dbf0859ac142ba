"""The pipelined main loop of the k-major x k-major weight-grad GEMM (gemm_x3p_impl.h, PIPE: the MFMA
fragments of K-step kt + 1 are read from LDS while step kt's MFMAs issue, and the LDS ring runs one step
later): K-step counts around the ring depth, tile edges, ensemble members and split-K slices, in split2h
through mtsac_debug_gemm_x3p_kmajor and (a subset) in split3 through mtsac_debug_gemm_x3p.  Every case is
held to |C - ref| <= 4e-6 |A|^T |B| against the float64 product of the same fp32 inputs (the bound of
test_gpu_x3p.py and test_split2h_products) and to bitwise equality with the unpipelined loop, which bit 16
of mtsac_debug_x3p_geo's ablation byte selects."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OLD_LOOP = 255 | (16 << 8)  # mtsac_debug_x3p_geo: geometry by operand form, ablation byte bit 16
RING = {2: 6, 3: 4}  # ring depth D in 16-deep K-steps: split2h, split3 (gemm_x3p_impl.h RING)
TILES = [(256, 128), (93, 136), (257, 132), (8, 8)]


def _ks(planes):
    """K = 32, 64, ... 16 (D + 2): 2 .. D + 2 K-steps around the ring depth; K = 1000 is padded to 1024."""
    return list(range(32, 16 * (RING[planes] + 2) + 1, 32)) + [1000]


def _cases(planes, tiles, members, slices):
    return [pytest.param(K, t, E, s, id=f"K{K}-{t[0]}x{t[1]}-E{E}-S{s}") for K in _ks(planes) for t in tiles
            for E in members for s in slices if s <= (K + 31) // 32]


@functools.lru_cache(maxsize=None)
def _operands(E, M, N, K):
    rng = np.random.default_rng(1000 * K + 10 * M + N + E)
    A = rng.standard_normal((E, K, M)).astype(np.float32)
    B = rng.standard_normal((E, K, N)).astype(np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    ref = np.einsum("ekm,ekn->emn", A64, B64)
    mag = np.einsum("ekm,ekn->emn", np.abs(A64), np.abs(B64))
    for x in (A, B, ref, mag):
        x.setflags(write=False)
    return A, B, ref, mag


def _run(planes, A, B, slices, old):
    from mtrl_amd import _lib as L

    lib = L.load()
    E, K, M = A.shape
    N = B.shape[2]
    C = np.zeros((E, M, N), np.float32)
    if old:
        lib.mtsac_debug_x3p_geo(OLD_LOOP)
    try:
        if planes == 2:
            L.check(lib.mtsac_debug_gemm_x3p_kmajor(E, M, N, K, slices, A.ctypes.data, B.ctypes.data, C.ctypes.data))
        else:
            assert E == 1
            L.check(lib.mtsac_debug_gemm_x3p(0 | (slices << 8), M, N, K, A.ctypes.data, 1, B.ctypes.data, 1,
                                             C.ctypes.data, None, None, None))
    finally:
        lib.mtsac_debug_x3p_geo(-1)
    return C


def _check(planes, K, tile, E, slices):
    A, B, ref, mag = _operands(E, tile[0], tile[1], K)
    C, C_old = _run(planes, A, B, slices, False), _run(planes, A, B, slices, True)
    err = np.abs(C.astype(np.float64) - ref)
    print("max |C - ref| / (|A|^T |B|):", float((err / mag).max()))
    assert np.all(err <= 4e-6 * mag), float((err / mag).max())
    assert np.array_equal(C.view(np.uint32), C_old.view(np.uint32))


@pytest.mark.parametrize("K, tile, E, slices", _cases(2, TILES, (1, 2), (1, 2, 3)))
def test_split2h_pipelined_loop(K, tile, E, slices):
    _check(2, K, tile, E, slices)


@pytest.mark.parametrize("K, tile, E, slices", _cases(3, [(256, 128), (257, 132)], (1,), (1, 2)))
def test_split3_pipelined_loop(K, tile, E, slices):
    _check(3, K, tile, E, slices)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("tile", [(93, 136), (257, 132)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_split2h_poisoned_output(tile, slices):
    """The entry's C starts as NaN between two guard bands: no NaN may remain inside [M, N], and the entry
    fails (naming the band) when a band was written."""
    A, B, ref, mag = _operands(2, tile[0], tile[1], 224)
    C = _run(2, A, B, slices, False)
    assert not np.isnan(C).any()
    assert np.all(np.abs(C - ref) <= 4e-6 * mag)
