// gradnorm.hip -- GradNorm's per-task losses and task-weight step over the per-task gradients (gfx950).
//
// The reference's optimizer (mtrl/optim/gradnorm.py) clips every task gradient to norm 1, latches the first
// per-task losses, forms the relative inverse training rates r_t, differentiates sum_t |n_t - mean(n) r_t^a|
// with respect to the T task weights, steps them with an inner [clip +] Adam, renormalises them to sum T and
// returns sum_t w_t g'_t.  The gradients enter only through the diagonal of G = M M^T (task_gram,
// pcgrad.hip), so the whole optimizer is T-vector algebra ending in T combine weights on the RAW rows,
// w_t s_t, and task_combine (pcgrad.hip) runs unchanged.  mtrl_amd/gradnorm.py (gradnorm_from_gram) is the
// host statement of this file, operation for operation.
//   * task_losses:    one wavefront, lane t sums task t's rows (i * T + t) in the order of i, in fp64.
//   * gradnorm_solve: one wavefront, lane t owns task t; fp64 arithmetic on the fp32 state, no contraction;
//                     every reduction over the tasks is the fixed shuffle tree of wave_sum, and the final
//                     renormalisation is in fp32 in the reference's order: (w / sum w) * T.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_sum.h"

namespace mtsac {
namespace {

__device__ inline float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// min that keeps a NaN (fmin drops it)
__device__ inline double wave_min_nan(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o);
    v = (v != v || u != u) ? nan("") : fmin(v, u);
  }
  return v;
}

// sign(0) = 0, NaN stays NaN
__device__ inline double sgn(double x) { return x != x ? x : (double)((x > 0.0) - (x < 0.0)); }

__global__ __launch_bounds__(64) void task_losses_kernel(const float* __restrict__ row, int T, int n, double inv,
                                                         float* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= T) return;
  // eight loads in flight, then their adds in the order of i: the sum is that of the plain loop, without a
  // memory latency per row
  double s = 0.0;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = row[(long long)(i + k) * T + t];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (double)v[k];
  }
  for (; i < n; ++i) s += (double)row[(long long)i * T + t];
  out[t] = (float)(s * inv);
}

__global__ __launch_bounds__(64) void task_losses_rows_kernel(const float* __restrict__ row_critic,
                                                              const float* __restrict__ row_actor,
                                                              const int* __restrict__ counts,
                                                              const int* __restrict__ rows, int max_rows, int T, int E,
                                                              float* __restrict__ out) {
  const int t = blockIdx.x, w = blockIdx.y, lane = threadIdx.x;
  const float* row = w == 0 ? row_critic : row_actor;
  const int n = min(counts[t], max_rows);
  const int* list = rows + (long long)t * max_rows;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += (double)row[list[j]];
  s = wave_sum(s);
  if (lane == 0) out[w * T + t] = n > 0 ? (float)(s / ((w == 0 ? (double)E : 1.0) * (double)n)) : 0.f;
}

__global__ __launch_bounds__(64) void gradnorm_solve_kernel(GradnormSolve s) {
#pragma clang fp contract(off)
  const int i = threadIdx.x, T = s.T;
  const bool on = i < T;
  const double* G = s.gram;
  const double dT = (double)T;
  // clip scales and clipped norms from the diagonal; |mean_t g_t| from the whole matrix
  const double gii = on ? G[i * T + i] : 0.0;
  const double nrm = sqrt(gii > 0.0 ? gii : 0.0);
  const double si = on ? (s.per_task_clip ? fmin(1.0, 1.0 / (nrm + 1e-8)) : 1.0) : 0.0;
  const double nt = si * nrm;
  double rowsum = 0.0;
  if (on)
    for (int k = 0; k < T; ++k) rowsum += G[i * T + k];
  const double total = wave_sum(rowsum);
  // latch, improvement, relative inverse rate
  const double L = on ? (double)s.losses[i] : 0.0;
  double L0 = on ? (double)s.original_losses[i] : 1.0;
  if (isinf(L0)) L0 = L;
  const double imp = on ? L / (L0 + 1e-12) : 0.0;
  const double r = imp / (wave_sum(imp) / dT + 1e-12);
  const double ra = on ? pow(r, s.asymmetry) : 0.0;  // NaN for r < 0, as jnp.power
  // the loss on the (weighted) norms and its gradient with respect to the weights
  const double w = on ? (double)s.task_weights[i] : 0.0;
  const double N = on ? (s.weighted ? fabs(w) * nt : nt) : 0.0;
  const double avg = wave_sum(N) / dT;
  const double d = on ? N - avg * ra : 0.0;
  const double loss = wave_sum(fabs(d));
  const double margin = wave_min_nan(on ? fabs(d) : INFINITY) / avg;
  double g = 0.0;  // reference form: the loss does not touch the weights
  if (s.weighted) {
    const double sg = sgn(d);
    const double c = wave_sum(on ? sg * ra : 0.0) / dT;
    g = on ? sgn(w) * nt * (sg - c) : 0.0;
  }
  // inner chain: [clip_by_global_norm,] Adam (b1 = 0.9, b2 = 0.999); count is the advanced one
  if (s.max_norm >= 0.0) {
    const double gn = sqrt(wave_sum(g * g));
    if (!(gn < s.max_norm)) g = (g / gn) * s.max_norm;
  }
  const double cnt = (double)s.count;
  const double mu = 0.9 * (on ? (double)s.mu[i] : 0.0) + (1.0 - 0.9) * g;
  const double nu = 0.999 * (on ? (double)s.nu[i] : 0.0) + (1.0 - 0.999) * g * g;
  const double upd = -s.lr * (mu / (1.0 - pow(0.9, cnt))) / (sqrt(nu / (1.0 - pow(0.999, cnt))) + s.eps);
  // apply and renormalise in fp32
  const float wn = on ? (float)(w + upd) : 0.f;
  const float sum = wave_sum_f(wn);
  const float wr = (wn / sum) * (float)T;
  if (on) {
    s.task_weights[i] = wr;
    s.original_losses[i] = (float)L0;
    s.mu[i] = (float)mu;
    s.nu[i] = (float)nu;
    s.w[i] = (float)((double)wr * si);
  }
  if (i == 0) {
    s.logs[0] = (float)loss;
    s.logs[1] = (float)margin;
    s.logs[5] = (float)(sqrt(total > 0.0 ? total : 0.0) / dT);
  }
}

}  // namespace

void task_losses(const float* row, int T, int n, double inv, float* out, hipStream_t st) {
  hipLaunchKernelGGL(task_losses_kernel, dim3(1), dim3(64), 0, st, row, T, n, inv, out);
}

void task_losses_rows(const float* row_critic, const float* row_actor, const int* counts, const int* rows,
                      int max_rows, int T, int E, float* out, hipStream_t st) {
  hipLaunchKernelGGL(task_losses_rows_kernel, dim3(T, 2), dim3(64), 0, st, row_critic, row_actor, counts, rows,
                     max_rows, T, E, out);
}

void gradnorm_solve(const GradnormSolve& s, hipStream_t st) {
  hipLaunchKernelGGL(gradnorm_solve_kernel, dim3(1), dim3(64), 0, st, s);
}

}  // namespace mtsac
