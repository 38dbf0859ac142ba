// pcgrad.hip -- PCGrad gradient surgery in Gram form over the per-task gradients (gfx950).
//
// The reference's optimizer (mtrl/optim/pcgrad.py:38-134) projects every task gradient g_i, in turn,
// off every g_j it conflicts with: T sequential passes over P-sized vectors per task.  Every projected
// gradient stays in the span of the task gradients, g_i^pc = sum_k C[i][k] g_k, so with the Gram matrix
// G = M M^T (M = the [T][P] per-task gradients) the whole surgery is T x T algebra:
//   D[i][:] = g_i^pc . g_: = C[i] G;  step j of row i:  proj = D[i][j] / (G[j][j] + 1e-8);
//   proj < 0:  C[i][j] -= proj,  D[i][:] -= proj G[j][:]
// and the update handed to the optimizer chain is mean_i g_i^pc = sum_k w_k g_k, w = mean_i C[i].
//   * task_gram:    G from M on v_mfma_f32_32x32x2_f32 (a lane's A and B operands of the diagonal blocks
//                   are the same register: M^T is never formed), fp32 over 64 columns, fp64 above that;
//                   one partial per workgroup, summed in fixed order;
//   * pcgrad_solve: one wavefront, fp64: the task order (pinned, or a Fisher-Yates draw from the engine's
//                   counter noise stream), the projections, w, the five PCGradState logs and the
//                   pre-surgery norm |mean_t g_t| = sqrt(sum_ij G_ij) / T;
//   * task_combine: out = sum_t w_t M[t] in the order t = 0..T-1 (no contraction: the fp32 ordered sum,
//                   bit for bit), streamed once, written at the padded leaf offsets of Net::g.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devrng.h"
#include "kernels.h"
#include "wave_sum.h"

namespace mtsac {
namespace {

constexpr int TP = 64;  // task rows padded (engine limit: 64 tasks)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16-byte streaming load (read once: no reuse to keep in the caches)
__device__ inline float4 load_stream4(const float* p) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// ------------------------------------------------------------------ Gram
// A workgroup owns columns [blockIdx.x * chunk, + chunk) (chunk a multiple of 256); its 4 waves take the
// chunk's 64-column tiles round robin.  Lane (r = lane & 31, h = lane >> 5) holds rows r and r + 32; of a
// tile it loads the float4s at columns 8u + 4h (u = 0..7), and every component is one MFMA step whose two
// k slots are the columns of the lanes' two halves.  Blocks (0,0), (0,1), (1,1) only: G is symmetric.
template <bool VEC>
__device__ inline void gram_tile_load(const float* __restrict__ M, int T, long long P, long long c0, long long cend,
                                      int row, int h, float4 (&v)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const long long c = c0 + 8 * u + 4 * h;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < T) {
      const float* p = M + (long long)row * P + c;
      if (VEC) {
        x = load_stream4(p);
      } else {
        if (c + 0 < cend) x.x = p[0];
        if (c + 1 < cend) x.y = p[1];
        if (c + 2 < cend) x.z = p[2];
        if (c + 3 < cend) x.w = p[3];
      }
    }
    v[u] = x;
  }
}

__global__ __launch_bounds__(256) void gram_kernel(const float* __restrict__ M, int T, long long P, long long chunk,
                                                   double* __restrict__ part /*[grid][TP*TP]*/) {
  __shared__ double red[TP * TP];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const bool two = T > 32;  // rows 32..63 in use
  const long long cb = (long long)blockIdx.x * chunk;
  const long long ce = cb + chunk < P ? cb + chunk : P;
  const bool aligned = (P & 3) == 0 && (reinterpret_cast<unsigned long long>(M) & 15) == 0;
  double t00[16], t01[16], t11[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) t00[i] = t01[i] = t11[i] = 0.0;
  for (long long c0 = cb + 64 * wave; c0 < ce; c0 += 256) {
    float4 a0[8], a1[8];
    if (aligned && c0 + 64 <= ce) {
      gram_tile_load<true>(M, T, P, c0, ce, r, h, a0);
      if (two) gram_tile_load<true>(M, T, P, c0, ce, r + 32, h, a1);
    } else {
      gram_tile_load<false>(M, T, P, c0, ce, r, h, a0);
      if (two) gram_tile_load<false>(M, T, P, c0, ce, r + 32, h, a1);
    }
    f32x16 c00 = {0}, c01 = {0}, c11 = {0};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float x0[4] = {a0[u].x, a0[u].y, a0[u].z, a0[u].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[q], x0[q], c00, 0, 0, 0);
      if (two) {
        const float x1[4] = {a1[u].x, a1[u].y, a1[u].z, a1[u].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[q], x1[q], c01, 0, 0, 0);
          c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[q], x1[q], c11, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      t00[i] += (double)c00[i];
      if (two) {
        t01[i] += (double)c01[i];
        t11[i] += (double)c11[i];
      }
    }
  }
  // the four waves' totals in wave order (deterministic); 32x32 C/D map: element i of lane (r, h) is
  // row (i & 3) + 8 (i >> 2) + 4 h, column r
  for (int i = tid; i < TP * TP; i += 256) red[i] = 0.0;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        red[row * TP + r] += t00[i];
        if (two) {
          red[row * TP + 32 + r] += t01[i];
          red[(32 + row) * TP + 32 + r] += t11[i];
        }
      }
    }
    __syncthreads();
  }
  double* out = part + (long long)blockIdx.x * TP * TP;
  for (int i = tid; i < TP * TP; i += 256) {
    const int a = i / TP, b = i % TP;
    out[i] = (a >= 32 && b < 32) ? red[b * TP + a] : red[i];
  }
}

// gram[i * T + j] = sum over the partials of part[p][i * TP + j]: one wave per entry, lane l takes partials
// l, l + 64, ... in order, then the lanes are summed in a fixed tree (deterministic)
__global__ __launch_bounds__(256) void gram_sum_kernel(const double* __restrict__ part, int nparts, int T,
                                                       double* __restrict__ gram) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= T * T) return;  // uniform over the wave
  const int i = k / T, j = k % T;
  double s = 0.0;
  for (int p = lane; p < nparts; p += 64) s += part[(long long)p * TP * TP + i * TP + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) gram[k] = s;
}

// ------------------------------------------------------------------ solve
// One wavefront; lane i owns row i of C and D (in the drawn order: row i is task perm[i]).
__global__ __launch_bounds__(64) void pcgrad_solve_kernel(PcgradSolve s) {
  __shared__ double D[TP][TP];  // [k][i]
  __shared__ double grow[TP];
  __shared__ int perm[TP];
  const int i = threadIdx.x, T = s.T;
  if (i == 0) {
    if (s.pinned) {
      for (int k = 0; k < T; ++k) perm[k] = s.pinned[k];
    } else {  // Fisher-Yates from the counter stream: draw k of this (network, step) is uniform4 row k / 4
      for (int k = 0; k < T; ++k) perm[k] = k;
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      int nd = 0;
      for (int k = T - 1; k > 0; --k, ++nd) {
        if ((nd & 3) == 0) uniform4(s.seed, s.stream_id, *s.counter, (uint32_t)(nd >> 2), u);
        int j = (int)(u[nd & 3] * (float)(k + 1));
        j = j > k ? k : j;
        const int tmp = perm[k];
        perm[k] = perm[j];
        perm[j] = tmp;
      }
    }
  }
  __syncthreads();
  const bool on = i < T;
  const int pi = on ? perm[i] : 0;
  if (on) s.perm_out[i] = pi;
  const double* G = s.gram;
  for (int k = 0; k < T; ++k) D[k][i] = on ? G[pi * T + perm[k]] : 0.0;
  const double gii = on ? G[pi * T + pi] : 0.0;
  double rowsum = 0.0;
  for (int k = 0; k < T; ++k) rowsum += D[k][i];
  double cos_before = 0.0;
  if (s.cosine_logs && on)
    for (int k = i + 1; k < T; ++k) {
      const double gkk = G[perm[k] * T + perm[k]];
      cos_before += D[k][i] / (sqrt(gii) * sqrt(gkk) + 1e-8);
    }
  double* C = s.ws_c;  // [k][i], global: row i is read back by its own lane only (until the cosine pass)
  int nconf = 0;
  for (int j = 0; j < T; ++j) {
    __syncthreads();
    grow[i] = on ? G[perm[j] * T + pi] : 0.0;  // G[j][i] of the ordered matrix (symmetric)
    __syncthreads();
    const double gjj = grow[j];
    double c = i == j ? 1.0 : 0.0;
    if (on) {
      const double proj = D[j][i] / (gjj + 1e-8);
      if (proj < 0.0) {
        ++nconf;
        c -= proj;
        for (int k = 0; k < T; ++k) D[k][i] -= proj * grow[k];
      }
    } else {
      c = 0.0;
    }
    C[j * TP + i] = c;
    const double colsum = wave_sum(c);  // sum_i C[i][j]
    if (i == 0) s.w[perm[j]] = (float)(colsum / (double)T);
  }
  double fii = 0.0;
  if (on)
    for (int k = 0; k < T; ++k) fii += C[k * TP + i] * D[k][i];
  const double mag_after = wave_sum(on ? sqrt(fii > 0.0 ? fii : 0.0) : 0.0) / (double)T;
  const double mag_before = wave_sum(on ? sqrt(gii) : 0.0) / (double)T;
  const double total = wave_sum(rowsum);
  const double confs = wave_sum((double)nconf) * 0.5;
  double cos_b = nan(""), cos_d = nan("");
  if (s.cosine_logs) {
    __syncthreads();  // every lane's C row is in memory
    // F[i][k] = g_i^pc . g_k^pc = sum_m D[m][i] C[m][k]
    __shared__ double fd[TP];
    fd[i] = fii;
    __syncthreads();
    double cos_after = 0.0;
    if (on)
      for (int k = i + 1; k < T; ++k) {
        double f = 0.0;
        for (int m = 0; m < T; ++m) f += D[m][i] * C[m * TP + k];
        const double ni = sqrt(fii > 0.0 ? fii : 0.0), nk = sqrt(fd[k] > 0.0 ? fd[k] : 0.0);
        cos_after += f / (ni * nk + 1e-8);
      }
    const double pairs = 0.5 * (double)T * (double)(T - 1) + 1e-8;
    cos_b = wave_sum(cos_before) / pairs;
    cos_d = cos_b - wave_sum(cos_after) / pairs;
  }
  if (i == 0) {
    s.logs[0] = (float)confs;
    s.logs[1] = (float)mag_after;
    s.logs[2] = (float)mag_before;
    s.logs[3] = (float)cos_b;
    s.logs[4] = (float)cos_d;
    s.logs[5] = (float)(sqrt(total > 0.0 ? total : 0.0) / (double)T);
  }
}

// ------------------------------------------------------------------ combine
template <bool VEC>
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ M, const float* __restrict__ w, int T,
                                                      long long P, PcgradLeaves lv, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float ws[TP];
  if (threadIdx.x < TP) ws[threadIdx.x] = threadIdx.x < T ? w[threadIdx.x] : 0.f;
  __syncthreads();
  constexpr int V = VEC ? 4 : 1;
  const long long n = (P + V - 1) / V;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const long long c = q * V;
    int k = 0;
    while (k + 1 < lv.n && c >= lv.dense[k + 1]) ++k;
    float* o = out + lv.padded[k] + (c - lv.dense[k]);
    if (VEC) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = 0; t < T; ++t) {
        const float4 m = load_stream4(M + (long long)t * P + c);
        const float wt = ws[t];
        acc.x = acc.x + wt * m.x;
        acc.y = acc.y + wt * m.y;
        acc.z = acc.z + wt * m.z;
        acc.w = acc.w + wt * m.w;
      }
      *reinterpret_cast<float4*>(o) = acc;
    } else {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = acc + ws[t] * M[(long long)t * P + c];
      *o = acc;
    }
  }
}

// ------------------------------------------------------------------ the step's extras
// logs[2] / logs[5]: the pre-surgery norms (the clip inside the optimizer saw the combined gradient's);
// logs[7]: mean explore loss (sum of the per-row terms / B)
__global__ __launch_bounds__(256) void pcgrad_logs_kernel(const float* __restrict__ solve_c,
                                                          const float* __restrict__ solve_a,
                                                          const float* __restrict__ row_e, int B,
                                                          float* __restrict__ logs) {
  __shared__ double sm[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) s += (double)row_e[b];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    logs[2] = solve_c[5];
    logs[5] = solve_a[5];
    logs[7] = (float)(sm[0] / (double)B);
  }
}

}  // namespace

int task_gram_parts(long long P, int max_parts) {
  return (int)std::max<long long>(1, std::min<long long>(max_parts, (P + 4095) / 4096));
}

void task_gram(const float* M, int T, long long P, int nparts, double* ws_part, double* gram, hipStream_t st) {
  long long chunk = (P + nparts - 1) / nparts;
  chunk = (chunk + 255) / 256 * 256;
  const int grid = (int)((P + chunk - 1) / chunk);  // <= nparts
  hipLaunchKernelGGL(gram_kernel, dim3(grid), dim3(256), 0, st, M, T, P, chunk, ws_part);
  hipLaunchKernelGGL(gram_sum_kernel, dim3((T * T + 3) / 4), dim3(256), 0, st, ws_part, grid, T, gram);
}

void pcgrad_solve(const PcgradSolve& s, hipStream_t st) {
  hipLaunchKernelGGL(pcgrad_solve_kernel, dim3(1), dim3(64), 0, st, s);
}

void task_combine(const float* M, const float* w, int T, long long P, const PcgradLeaves& lv, float* out,
                  hipStream_t st) {
  bool vec = (P & 3) == 0 && (reinterpret_cast<unsigned long long>(M) & 15) == 0 &&
             (reinterpret_cast<unsigned long long>(out) & 15) == 0;
  for (int k = 0; k < lv.n; ++k) vec = vec && (lv.dense[k] & 3) == 0 && (lv.padded[k] & 3) == 0;
  const long long n = vec ? P / 4 : P;
  const int grid = (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 4096));
  if (vec) hipLaunchKernelGGL((combine_kernel<true>), dim3(grid), dim3(256), 0, st, M, w, T, P, lv, out);
  else hipLaunchKernelGGL((combine_kernel<false>), dim3(grid), dim3(256), 0, st, M, w, T, P, lv, out);
}

void pcgrad_logs(const float* solve_critic, const float* solve_actor, const float* row_explore, int B, float* logs,
                 hipStream_t st) {
  hipLaunchKernelGGL(pcgrad_logs_kernel, dim3(1), dim3(256), 0, st, solve_critic, solve_actor, row_explore, B, logs);
}

}  // namespace mtsac
