// cagrad.hip -- CAGrad's weight search in Gram form over the per-task gradients (gfx950).
//
// The reference's optimizer (mtrl/optim/cagrad.py) clips every task gradient to norm 1, searches T task
// weights by momentum SGD on an objective that sees the gradients only through their Gram matrix, and
// returns sum_t (1/T + tw_t lambda) g'_t / (1 + c^2).  With G = M M^T (task_gram, pcgrad.hip) the clip is
// G' = diag(s) G diag(s), s_t = min(1, 1 / (sqrt(G_tt) + 1e-8)), and the whole optimizer is T x T algebra
// that ends in T combine weights on the RAW rows, w_t = s_t (1/T + tw_t lambda) / (1 + c^2): task_combine
// (pcgrad.hip) then runs unchanged.  mtrl_amd/cagrad.py (cagrad_from_gram) is the host statement of this
// file, operation for operation.
//   * cagrad_solve: one wavefront, fp64, no contraction.  Lane i owns task i: row i of GG in LDS (stored
//                   [k][i], so the lanes of one read hit 64 consecutive doubles), w_i, v_i and w_best_i in
//                   registers.  Every reduction over the tasks is the fixed shuffle tree of wave_sum;
//                   lanes at or above T hold exact zeros.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_sum.h"

namespace mtsac {
namespace {

constexpr int TP = 64;  // task rows padded (engine limit: 64 tasks)

__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(64) void cagrad_solve_kernel(CagradSolve s) {
#pragma clang fp contract(off)
  __shared__ double GG[TP][TP];  // [k][i]: entry (i, k) of the clipped, scaled Gram matrix
  __shared__ double vec[TP];     // the vector of the current matrix-vector product
  __shared__ double pd[TP];      // diag(G')
  const int i = threadIdx.x, T = s.T;
  const bool on = i < T;
  const double* G = s.gram;
  const double dT = (double)T;
  // clip scales from the diagonal; G' = diag(s) G diag(s)
  const double gii = on ? G[i * T + i] : 0.0;
  const double si = on ? fmin(1.0, 1.0 / (sqrt(gii > 0.0 ? gii : 0.0) + 1e-8)) : 0.0;
  vec[i] = si;
  __syncthreads();
  double rowsum = 0.0;  // of the raw matrix: |mean_t g_t|^2 T^2 summed over the lanes
  for (int k = 0; k < TP; ++k) {
    const double g = (on && k < T) ? G[i * T + k] : 0.0;
    rowsum += g;
    GG[k][i] = si * g * vec[k];
  }
  const double pii = GG[i][i];
  pd[i] = pii;
  __syncthreads();
  const double ni = sqrt(pii > 0.0 ? pii : 0.0);
  const double before = wave_sum(on ? ni : 0.0) / dT;
  double cosv = nan("");
  if (s.cosine_logs) {
    double cs = 0.0;
    if (on)
      for (int k = i + 1; k < T; ++k) {
        const double pk = pd[k];
        cs += GG[k][i] / (ni * sqrt(pk > 0.0 ? pk : 0.0) + 1e-8);
      }
    cosv = wave_sum(cs) / (0.5 * dT * (double)(T - 1) + 1e-8);
  }
  // scaling: GG = G' / scale^2, Gg = row means, gg = their mean, c_n = c sqrt(gg + 1e-4)
  const double scale = wave_sum(on ? sqrt(pii + 1e-4) : 0.0) / dT;
  const double sc2 = scale * scale;
  double Gg = 0.0;
  for (int k = 0; k < T; ++k) {
    const double x = GG[k][i] / sc2;
    GG[k][i] = x;
    Gg += x;
  }
  Gg = Gg / dT;
  const double gg = wave_sum(Gg) / dT;
  const double c_n = s.c * sqrt(gg + 1e-4);
  // the search: iters - 1 momentum-SGD steps, every iterate (the last one too) evaluated, the first
  // iterate of the lowest objective kept
  double w = (on && s.w0) ? s.w0[i] : 0.0;
  double v = 0.0, w_best = w, obj_best = INFINITY;
  int best_it = -1;
  for (int it = 0; it < s.iters; ++it) {
    const double S = wave_sum(w) + 1e-8;
    const double ww = on ? w / S : 0.0;
    __syncthreads();
    vec[i] = ww;
    __syncthreads();
    double Gw = 0.0;
    for (int k = 0; k < T; ++k) Gw += GG[k][i] * vec[k];
    const double rq = sqrt(wave_sum(ww * Gw) + 1e-4);
    const double obj = wave_sum(ww * Gg) + c_n * rq;
    const double u = Gg + c_n * Gw / rq;
    const double wu = wave_sum(ww * u);
    const double grad = on ? (u - wu) / S : 0.0;
    if (i == 0) s.obj_hist[it] = obj;
    if (obj < obj_best) {  // uniform over the wave
      obj_best = obj;
      w_best = w;
      best_it = it;
    }
    if (it + 1 < s.iters) {
      v = s.momentum * v + grad;
      w = w - s.lr * v;
    }
  }
  // task_weights = softmax(w_best); lambda; the combine weights on the raw rows
  const double m = wave_max(on ? w_best : -INFINITY);
  const double e = on ? exp(w_best - m) : 0.0;
  const double tw = e / wave_sum(e);
  __syncthreads();
  vec[i] = tw;
  __syncthreads();
  double Gt = 0.0;
  for (int k = 0; k < T; ++k) Gt += GG[k][i] * vec[k];
  const double gw = sqrt(wave_sum(tw * Gt) + 1e-4);
  const double lam = c_n / (gw + 1e-4);
  const double wc = si * (1.0 / dT + tw * lam) / (1.0 + s.c * s.c);
  // |combined| = sqrt(w^T G w) on the raw matrix
  __syncthreads();
  vec[i] = wc;
  __syncthreads();
  double r = 0.0;
  if (on)
    for (int k = 0; k < T; ++k) r += G[i * T + k] * vec[k];
  const double mag2 = wave_sum(wc * r);
  const double total = wave_sum(rowsum);
  if (on) {
    s.w[i] = (float)wc;
    s.task_weights[i] = (float)tw;
  }
  if (i == 0) {
    s.logs[0] = (float)sqrt(mag2 > 0.0 ? mag2 : 0.0);
    s.logs[1] = (float)before;
    s.logs[2] = (float)cosv;
    s.logs[3] = (float)obj_best;
    s.logs[4] = (float)best_it;
    s.logs[5] = (float)(sqrt(total > 0.0 ? total : 0.0) / dT);
  }
}

}  // namespace

void cagrad_solve(const CagradSolve& s, hipStream_t st) {
  hipLaunchKernelGGL(cagrad_solve_kernel, dim3(1), dim3(64), 0, st, s);
}

}  // namespace mtsac
