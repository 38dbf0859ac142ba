// symeig.hip -- all eigenvalues of Z dense symmetric fp64 matrices of one order r (gfx950), for the srank of
// the activation Grams (netmetrics.hip): Householder reduction to tridiagonal form, then Sturm-count bisection.
// Eigenvalues only; evaluation time only.  DESIGN.md section 19.
//
// sym_tridiag (in place on A [Z][r][r], both triangles stored, bitwise symmetric).  Column k = 0 .. r - 1, with
// m = r - k - 1 rows below the diagonal, is two launches, and the rank-2 update of column k - 1 is still
// pending when it starts (v', p' and the partial sums of p'^T v' are in the other slot of the scratch):
//   head   one workgroup per matrix.  c' = (tau' / 2) p'^T v' from the partials in one fixed order (strided per
//          thread, LDS tree), w' = p' - c' v' stored over p'.  Row k of the updated matrix is formed on the fly,
//          a_kj - (v'_0 w'_j + w'_0 v'_j), and never stored.  d_k = its first entry, x = the rest (= column k
//          below the diagonal); tail = sum_{i >= 1} x_i^2 by per-thread strided sums and the LDS tree;
//          tail == 0: no reflection (tau = 0, e_k = x_0); else alpha = -sign(x_0) sqrt(x_0^2 + tail),
//          e_k = alpha, v = (1, x_1 / (x_0 - alpha), ...), tau = (alpha - x_0) / alpha, so
//          (I - tau v v^T) x = alpha e_1.
//   sweep  (m >= 1) one pass over A[k+1:, k+1:]: a workgroup owns SE_ROWS whole rows, a wavefront two of them.
//          Lane l walks columns l, l + 64, ...: A_ij = A_ij - (v'_i w'_j + w'_i v'_j) is stored and its new
//          value goes into the row's sum for p = tau A v (ascending per lane, then the xor-shuffle tree).  The
//          workgroup leaves the sum of its rows' p_i v_i (ascending) in part[band].
// These are the two fusions the unblocked reduction allows: correction and update share a launch, and the next
// column's reflector and product read the freshly updated values, so the trailing block is read and written
// once per column.  Ordering comes from the stream alone: no float atomics, no cooperative launch, no
// workgroup waits on another.  Every sum has one order fixed by (r, k), and every grid is per matrix, so a
// matrix's result is bitwise the same alone and inside any batch.
// Symmetry: both triangles are updated.  The file is compiled with floating-point contraction off, so
// v_i w_j + w_i v_j is two rounded products and one sum; products and the sum commute and w is stored once,
// so element (i, j) and element (j, i) get the same bits.
//
// tridiag_eigvals: thread j bisects for the j-th eigenvalue (ascending) with the Sturm count of LAPACK's
// dlaebz, q_i = d_i - x - e_{i-1}^2 / q_{i-1} with |q| <= pivmin replaced by -pivmin, which is monotone in x
// in IEEE arithmetic: the r bisections walk one tree of midpoints and stay ordered.  Start: the Gershgorin
// interval widened by 2 r 2^-52 |T| + 2 pivmin; SE_HALVINGS halvings whatever the data, so the kernel ends on
// any input.  All lanes read the same (d_i, e_{i-1}^2) at the same time: the pairs are staged in LDS (16 r
// bytes, r <= SYM_EIG_MAX_ORDER = 8192) and read as broadcasts; measured against wave-uniform global loads,
// one pair per step and in chunks of 8 fetched a chunk ahead.
// A matrix with |T| = 0 gives 0.0 exactly; a matrix with a non-finite entry (flag bit 0) or a non-finite
// tridiagonal form (bit 1) gives NaN for every j.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "kernels.h"
#include "wave_sum.h"

#pragma clang fp contract(off)

namespace mtsac {
namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_ROWS = 8;       // rows of a sweep workgroup (two per wavefront)
constexpr int SE_HALVINGS = 64;  // 2 |T| 2^-64 is far below 2^-52 |T|
constexpr int SE_SCAN_BLOCKS = 64;

// deterministic block sum (a tree over LDS: the same order whatever the schedule)
__device__ inline double se_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = SE_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// flags[z] bit 0: the matrix holds a non-finite entry (integer atomic; flags zeroed before)
__global__ __launch_bounds__(SE_THREADS) void sym_scan_kernel(const double* __restrict__ A, long long n,
                                                              int* __restrict__ flags) {
  const int z = blockIdx.y;
  const double* Az = A + (long long)z * n;
  int bad = 0;
  for (long long i = (long long)blockIdx.x * SE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SE_THREADS)
    bad |= isfinite(Az[i]) ? 0 : 1;
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&flags[z], 1);
}

// Column k, first launch: one workgroup per matrix.  Finishes the pending reflection of column k - 1 (c, then
// w = p - c v in place of p), forms row k of the updated matrix on the fly (never stored: nothing reads it
// again), and from it d_k and the reflector of column k.  v, p: [2][Z][r], column k's in slot k & 1.
__global__ __launch_bounds__(SE_THREADS) void sym_head_kernel(const double* __restrict__ A, int r, int k, int Z,
                                                              double* __restrict__ d, double* __restrict__ e,
                                                              double* v, double* p, const double* __restrict__ part,
                                                              int parts, double* tau) {
  __shared__ double red[SE_THREADS];
  const int z = blockIdx.x, tid = threadIdx.x;
  const int cur = k & 1, prv = cur ^ 1;
  const int m = r - k - 1;
  // the pending block is A[k:, k:], m + 1 rows: vp, wp are indexed from row k
  const double tp = k > 0 ? tau[prv * Z + z] : 0.0;
  const double* vp = v + ((long long)prv * Z + z) * r;
  double* wp = p + ((long long)prv * Z + z) * r;
  if (tp != 0.0) {  // a NaN tau takes this branch and spreads
    const int nb = (m + 1 + SE_ROWS - 1) / SE_ROWS;
    double s = 0.0;
    for (int b = tid; b < nb; b += SE_THREADS) s += part[(long long)z * parts + b];
    const double c = (0.5 * tp) * se_block_sum(s, red);
    for (int i = tid; i <= m; i += SE_THREADS) wp[i] = wp[i] - c * vp[i];
    __syncthreads();
  }
  const double* row = A + ((long long)z * r + k) * r + k;
  const double v0p = tp != 0.0 ? vp[0] : 0.0, w0p = tp != 0.0 ? wp[0] : 0.0;
  auto at = [&](int j) { return tp != 0.0 ? row[j] - (v0p * wp[j] + w0p * vp[j]) : row[j]; };
  if (tid == 0) d[(long long)z * r + k] = at(0);
  if (m == 0) return;
  double s = 0.0;
  for (int i = 1 + tid; i < m; i += SE_THREADS) {
    const double xi = at(1 + i);
    s += xi * xi;
  }
  const double tail = se_block_sum(s, red);
  const double x0 = at(1);
  double alpha = x0, t = 0.0, v0 = 1.0;
  if (tail != 0.0) {  // a NaN tail takes this branch and spreads
    alpha = -copysign(sqrt(x0 * x0 + tail), x0);
    t = (alpha - x0) / alpha;
    v0 = x0 - alpha;
  }
  double* vz = v + ((long long)cur * Z + z) * r;
  for (int i = 1 + tid; i < m; i += SE_THREADS) vz[i] = at(1 + i) / v0;
  if (tid == 0) {
    vz[0] = 1.0;
    e[(long long)z * (r - 1) + k] = alpha;
    tau[cur * Z + z] = t;
  }
}

// Column k, second launch, m >= 1: one pass over the trailing block A[k+1:, k+1:].  Applies the pending
// reflection of column k - 1, A_ij = A_ij - (v'_i w'_j + w'_i v'_j), stores it, and adds the new values into
// p = tau A v of column k.  A workgroup owns SE_ROWS whole rows, a wavefront two of them.
__global__ __launch_bounds__(SE_THREADS) void sym_sweep_kernel(double* __restrict__ A, int r, int k, int Z,
                                                               const double* v, double* p,
                                                               double* __restrict__ part, int parts,
                                                               const double* __restrict__ tau) {
  __shared__ double pv[SE_ROWS];
  const int z = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cur = k & 1, prv = cur ^ 1;
  const double tn = tau[cur * Z + z], tp = k > 0 ? tau[prv * Z + z] : 0.0;
  if (tn == 0.0 && tp == 0.0) return;  // nothing pending and no reflection: the block stays as it is
  const bool pend = tp != 0.0, refl = tn != 0.0;
  const int m = r - k - 1;
  double* Az = A + (long long)z * r * r + (long long)(k + 1) * r + (k + 1);
  const double* vp = v + ((long long)prv * Z + z) * r + 1;  // from row k + 1 on
  const double* wp = p + ((long long)prv * Z + z) * r + 1;
  const double* vz = v + ((long long)cur * Z + z) * r;
  const int i0 = blockIdx.x * SE_ROWS + 2 * wave, i1 = i0 + 1;
  const bool ok0 = i0 < m, ok1 = i1 < m;
  const int c0 = min(i0, m - 1), c1 = min(i1, m - 1);  // a row past the end reads a valid one, stores nothing
  double* R0 = Az + (long long)c0 * r;
  double* R1 = Az + (long long)c1 * r;
  const double v0 = pend ? vp[c0] : 0.0, w0 = pend ? wp[c0] : 0.0;
  const double v1 = pend ? vp[c1] : 0.0, w1 = pend ? wp[c1] : 0.0;
  double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
  for (int j = lane; j < m; j += 64) {
    double x0 = R0[j], x1 = R1[j];
    if (pend) {
      const double vj = vp[j], wj = wp[j];
      x0 = x0 - (v0 * wj + w0 * vj);
      x1 = x1 - (v1 * wj + w1 * vj);
      if (ok0) R0[j] = x0;
      if (ok1) R1[j] = x1;
    }
    if (refl) {
      const double vj = vz[j];
      a0 += x0 * vj;
      a1 += x1 * vj;
    }
  }
  if (!refl) return;
  a0 = tn * wave_sum(a0);
  a1 = tn * wave_sum(a1);
  if (lane == 0) {
    double* pz = p + ((long long)cur * Z + z) * r;
    if (ok0) pz[i0] = a0;
    if (ok1) pz[i1] = a1;
    pv[2 * wave] = ok0 ? a0 * vz[i0] : 0.0;
    pv[2 * wave + 1] = ok1 ? a1 * vz[i1] : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < SE_ROWS; ++q) s += pv[q];
    part[(long long)z * parts + blockIdx.x] = s;
  }
}

// number of eigenvalues of the tridiagonal matrix below x (dlaebz's recurrence); de[i] = (d_i, e_{i-1}^2) in LDS,
// every lane reads the same word (a broadcast, no bank conflict)
__device__ inline int sturm_count(const double2* de, int r, double x, double pivmin) {
  double q = de[0].x - x;
  if (fabs(q) <= pivmin) q = -pivmin;
  int cnt = q <= 0.0 ? 1 : 0;
#pragma unroll 8
  for (int i = 1; i < r; ++i) {
    const double2 t = de[i];
    q = t.x - x - t.y / q;
    if (fabs(q) <= pivmin) q = -pivmin;
    cnt += q <= 0.0 ? 1 : 0;
  }
  return cnt;
}

__global__ __launch_bounds__(64) void tridiag_eigvals_kernel(const double* __restrict__ d,
                                                             const double* __restrict__ e, int r,
                                                             double* __restrict__ lam, int* flags) {
  extern __shared__ double2 de[];  // [r]
  const int z = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  const double* dz = d + (long long)z * r;
  const double* ez = e + (long long)z * (r - 1);
  for (int i = threadIdx.x; i < r; i += 64) {
    const double ei = i > 0 ? ez[i - 1] : 0.0;
    de[i] = double2{dz[i], ei * ei};
  }
  __syncthreads();
  double gl = dz[0], gu = dz[0], emax2 = 0.0;
  bool finite = true;
  for (int i = 0; i < r; ++i) {
    const double el = i > 0 ? fabs(ez[i - 1]) : 0.0, er = i < r - 1 ? fabs(ez[i]) : 0.0;
    const double c = dz[i], rad = el + er, e2 = er * er;
    finite = finite && isfinite(c) && isfinite(rad) && isfinite(e2);
    gl = fmin(gl, c - rad);
    gu = fmax(gu, c + rad);
    emax2 = fmax(emax2, e2);
  }
  if (j >= r) return;
  double* out = lam + (long long)z * r + j;
  if (!finite || (flags[z] & 1)) {  // bit 0 was set before this launch; bit 1 has this one writer
    *out = __builtin_nan("");
    if (j == 0 && !finite) flags[z] |= 2;
    return;
  }
  const double tnorm = fmax(fabs(gl), fabs(gu));
  if (tnorm == 0.0) {
    *out = 0.0;
    return;
  }
  const double pivmin = DBL_MIN * fmax(1.0, emax2);
  const double wide = 2.0 * tnorm * 0x1p-52 * (double)r + 2.0 * pivmin;
  double lo = gl - wide, hi = gu + wide;
  for (int it = 0; it < SE_HALVINGS; ++it) {
    const double mid = 0.5 * lo + 0.5 * hi;
    if (sturm_count(de, r, mid, pivmin) >= j + 1)
      hi = mid;
    else
      lo = mid;
  }
  *out = 0.5 * lo + 0.5 * hi;
}

}  // namespace

int sym_tridiag_parts(int r) { return std::max(1, (r + SE_ROWS - 1) / SE_ROWS); }

int sym_tridiag_launches(int r) { return 2 + r + (r - 1); }

void sym_tridiag(const SymEig& s, hipStream_t st) {
  const int r = s.r, parts = sym_tridiag_parts(r);
  (void)hipMemsetAsync(s.flags, 0, sizeof(int) * s.Z, st);
  const long long n = (long long)r * r;
  const int scan_blocks = (int)std::min<long long>(SE_SCAN_BLOCKS, (n + SE_THREADS - 1) / SE_THREADS);
  hipLaunchKernelGGL(sym_scan_kernel, dim3(scan_blocks, s.Z), dim3(SE_THREADS), 0, st, s.A, n, s.flags);
  for (int k = 0; k < r; ++k) {
    const int m = r - k - 1;
    hipLaunchKernelGGL(sym_head_kernel, dim3(s.Z), dim3(SE_THREADS), 0, st, s.A, r, k, s.Z, s.d, s.e, s.v, s.p, s.part,
                       parts, s.tau);
    if (m >= 1)
      hipLaunchKernelGGL(sym_sweep_kernel, dim3((m + SE_ROWS - 1) / SE_ROWS, s.Z), dim3(SE_THREADS), 0, st, s.A, r, k,
                         s.Z, s.v, s.p, s.part, parts, s.tau);
  }
}

void tridiag_eigvals(const SymEig& s, hipStream_t st) {
  const size_t lds = sizeof(double2) * s.r;  // <= 128 KiB of the CU's 160 KiB at SYM_EIG_MAX_ORDER
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)tridiag_eigvals_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(tridiag_eigvals_kernel, dim3((s.r + 63) / 64, s.Z), dim3(64), lds, st, s.d, s.e, s.r, s.lam,
                     s.flags);
}

}  // namespace mtsac
