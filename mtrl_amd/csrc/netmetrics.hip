// netmetrics.hip -- network health metrics of the trunk activations (gfx950): the dormant-neuron
// statistics and the Gram matrix the feature rank (srank) is computed from.  Evaluation time only.
//
// Both kernels read Z fp32 matrices H[z] of M rows x W columns (row stride ld, matrix stride sH): the
// post-ReLU outputs of one trunk layer for the Z ensemble members, over the M real batch rows.
//   * act_stats: s_j = mean_b |H[b][j]| with the column sums accumulated in fp64 (one partial per row
//     chunk, then a finish that adds the chunks in order), the layer mean of s, the normalised score
//     s~_j = s_j / (mean_j s_j + 1e-9) and the number of neurons with s~_j <= threshold.  No float atomics:
//     every sum has one fixed order, so the outputs are bitwise equal run to run.
//   * act_gram: G = H^T H (W x W) when W <= M, else G = H H^T (M x M), in fp64 on the matrix cores
//     (v_mfma_f64_16x16x4_f64).  The fp32 inputs are widened on load, so every product is exact and the
//     only error is the fp64 accumulation over the summed dimension.  A workgroup owns one 64 x 64 tile of
//     the upper triangle over the whole summed dimension (no split: one fixed order) and stores every
//     element at (i, j) and (j, i): G is bitwise symmetric.  The singular values of H are the square roots
//     of G's eigenvalues (host: mtrl_amd/netmetrics.py).
// The f64 MFMA's lane maps: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; of
// its four results, register q is D[i = (l >> 4) + 4 q][j = l & 15] -- not the row map of the f32 forms.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace mtsac {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_CHUNKS = 64;
constexpr int ST_CHUNK_ROWS = 64;  // rows a chunk holds at least (fewer chunks for short matrices)

// part[z][c][w] = sum over the rows of chunk c of |H[z][row][w]|, rows in ascending order
__global__ __launch_bounds__(ST_THREADS) void act_colabs_kernel(const float* __restrict__ H, int M, int W, int ld,
                                                                  long long sH, int chunk_rows, int chunks,
                                                                  double* __restrict__ part) {
  const int w = blockIdx.x * ST_THREADS + threadIdx.x;
  const int c = blockIdx.y, z = blockIdx.z;
  if (w >= W) return;
  const int r0 = c * chunk_rows;
  const int r1 = min(M, r0 + chunk_rows);
  const float* p = H + (long long)z * sH + (long long)r0 * ld + w;
  double acc = 0.0;
#pragma unroll 4
  for (int r = r0; r < r1; ++r, p += ld) acc += (double)fabsf(*p);
  part[((long long)z * chunks + c) * W + w] = acc;
}

// deterministic block sums (a tree over LDS: the same order whatever the schedule)
__device__ inline double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// one workgroup per matrix: s (fp32), the mean of s over the columns, s~ and the dormant count
__global__ __launch_bounds__(ST_THREADS) void act_stats_finish_kernel(const double* __restrict__ part, int M, int W,
                                                                        int chunks, float threshold,
                                                                        float* __restrict__ score, long long s_score,
                                                                        float* __restrict__ norm, long long s_norm,
                                                                        int* __restrict__ count, int s_count) {
  __shared__ double red[ST_THREADS];
  const int z = blockIdx.x, tid = threadIdx.x;
  const double* pz = part + (long long)z * chunks * W;
  float* sc = score + (long long)z * s_score;
  float* nr = norm + (long long)z * s_norm;
  double local = 0.0;
  for (int j = tid; j < W; j += ST_THREADS) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += pz[(long long)c * W + j];
    s /= (double)M;
    sc[j] = (float)s;
    local += s;
  }
  const double mean = block_sum(local, red) / (double)W;
  const float den = (float)(mean + 1e-9);
  int dormant = 0;
  for (int j = tid; j < W; j += ST_THREADS) {
    const float v = sc[j] / den;  // this thread's own store above
    nr[j] = v;
    dormant += v <= threshold ? 1 : 0;
  }
  const double total = block_sum((double)dormant, red);  // whole numbers below 2^53: exact
  if (tid == 0) count[(long long)z * s_count] = (int)total;
}

// ------------------------------------------------------------------ fp64 Gram
constexpr int GT = 64;    // output tile (rows and columns of G)
constexpr int GK = 16;    // summed-dimension step through LDS
constexpr int GLD = 80;   // LDS row stride (doubles): the four k rows of a wave read land on disjoint banks

// element (k, i) of the operand: H[k][i] (side 0, G = H^T H) or H[i][k] (side 1, G = H H^T)
__global__ __launch_bounds__(256) void act_gram_kernel(const float* __restrict__ H, int ld, long long sH, int side,
                                                       int r, int K, int nt, double* __restrict__ G, long long sG) {
  __shared__ double As[GK * GLD];
  __shared__ double Bs[GK * GLD];
  int t = blockIdx.x, ti = 0;
  while (t >= nt - ti) {
    t -= nt - ti;
    ++ti;
  }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const float* Hz = H + (long long)blockIdx.y * sH;
  double* Gz = G + (long long)blockIdx.y * sG;
  const long long sk = side == 0 ? ld : 1, si = side == 0 ? 1 : ld;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const bool live = !diag || wc >= wr;  // a diagonal tile's lower quadrant is the upper one's mirror
  const int l15 = lane & 15, l4 = lane >> 4;
  const double* Bp = diag ? As : Bs;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
    for (int u = 0; u < GT * GK / 256; ++u) {
      const int e = tid + 256 * u;
      const int kk = side == 0 ? e >> 6 : e & (GK - 1);
      const int ii = side == 0 ? e & (GT - 1) : e >> 4;
      const int k = k0 + kk;
      const int ia = ti * GT + ii, ib = tj * GT + ii;
      As[kk * GLD + ii] = (k < K && ia < r) ? (double)Hz[(long long)k * sk + (long long)ia * si] : 0.0;
      if (!diag) Bs[kk * GLD + ii] = (k < K && ib < r) ? (double)Hz[(long long)k * sk + (long long)ib * si] : 0.0;
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int kq = 0; kq < GK; kq += 4) {
        const int kk = kq + l4;
        const double a0 = As[kk * GLD + wr * 32 + l15], a1 = As[kk * GLD + wr * 32 + 16 + l15];
        const double b0 = Bp[kk * GLD + wc * 32 + l15], b1 = Bp[kk * GLD + wc * 32 + 16 + l15];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = ti * GT + wr * 32 + a * 16 + l4 + 4 * q;
        const int col = tj * GT + wc * 32 + b * 16 + l15;
        if (row >= r || col >= r || col < row) continue;
        const double v = acc[a][b][q];
        Gz[(long long)row * r + col] = v;
        Gz[(long long)col * r + row] = v;
      }
}

}  // namespace

int act_stats_chunks(int M) { return std::max(1, std::min(ST_MAX_CHUNKS, (M + ST_CHUNK_ROWS - 1) / ST_CHUNK_ROWS)); }

void act_stats(const ActStats& s, hipStream_t st) {
  const int chunks = act_stats_chunks(s.M);
  const int chunk_rows = (s.M + chunks - 1) / chunks;
  const dim3 grid((s.W + ST_THREADS - 1) / ST_THREADS, chunks, s.Z);
  hipLaunchKernelGGL(act_colabs_kernel, grid, dim3(ST_THREADS), 0, st, s.H, s.M, s.W, s.ld, s.sH, chunk_rows, chunks,
                     s.part);
  hipLaunchKernelGGL(act_stats_finish_kernel, dim3(s.Z), dim3(ST_THREADS), 0, st, s.part, s.M, s.W, chunks, s.threshold,
                     s.score, s.s_score, s.norm, s.s_norm, s.count, s.s_count);
}

int act_gram_dim(int M, int W) { return std::min(M, W); }

void act_gram(const ActGram& g, hipStream_t st) {
  const int side = g.W <= g.M ? 0 : 1;
  const int r = act_gram_dim(g.M, g.W), K = side == 0 ? g.M : g.W;
  const int nt = (r + GT - 1) / GT;
  hipLaunchKernelGGL(act_gram_kernel, dim3(nt * (nt + 1) / 2, g.Z), dim3(256), 0, st, g.H, g.ld, g.sH, side, r, K, nt,
                     g.gram, g.sG);
}

}  // namespace mtsac
