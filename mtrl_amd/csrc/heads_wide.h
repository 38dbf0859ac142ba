// heads_wide.h -- the head kernels for wide heads (hd > 8, action_dim 5 .. 64): the policy head forward,
// the head backward (data and weights) and the action grad as per-task grouped GEMMs on the f32-input
// MFMA v_mfma_f32_16x16x4_f32.  Included by heads.hip inside its unnamed namespace (it uses wsum,
// softplusf, clip_grad, head_bwd_put and the constants defined there).
//
// The instruction's result is bitwise a k-ordered fmaf chain (one rounding per product, no wider
// accumulator), and row i of its output reads row i of the A operand only: a row's outputs cannot
// depend on which other rows share its tile, and every sum below has ONE order, fixed by the shape.
// Operand maps (lane l): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; C/D register v of lane l
// is element [4 (l >> 4) + v][l & 15].
//
// Nothing is sized by hd: the outputs are walked in 16-wide tiles, NT of them per wave (NT in 1, 2, 4,
// 8: the only template parameter; hd <= 128 = 16 * 8), LDS holds 16-row tiles at that fixed width.
// All widths are multiples of 4 (the engine creates no others; the launch wrappers refuse the rest).

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WIDE_MAX_HD = 128;
constexpr int WIDE_KS = 4;  // waves of a forward / action-grad workgroup = partial sums of one output

// how many 16-wide output tiles a wave carries for nout outputs: the instance NT >= ceil(nout / 16)
inline int wide_nt(int nout) {
  const int tiles = (nout + 15) / 16;
  return tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
}

// acc[c][.] += A (16 x K) * B (K x nout), output tile c = outputs 16 c .. 16 c + 15.
// ar: this lane's A row (row l & 15 of the tile), K contiguous floats, or null: a row of zeros.
// B either k-contiguous (KT: B[o * K + k], the transposed head kernel WhT, the critic's layer-0 rows) or
// output-contiguous (B[k * nout + o]: Wh); the operand values are the same, so are the bits.
// SUMMATION ORDER of one output (row r, output o): WIDE_KS = 4 partial sums, one per wave g of the workgroup,
// each a single fmaf chain over its 16-k blocks k0 = 16 (g + 4 i), i = 0, 1, ...:
//   for k0 = 16 g, 16 g + 64, ...: for s = 0 .. 3: for kk = 0 .. 3: k = k0 + 4 kk + s
// (lane (i, kk) loads A[i][k0 + 4 kk .. + 3] with one 16-B load and feeds element s to the block's s-th
// MFMA, whose own chain runs over kk; past K the chain adds exact zeros), then ((P0 + P1) + P2) + P3.
// The split is the same at every K (a wave without blocks holds zeros): fixed by the shape alone.
// one 16-k block's operands of this lane (zeros past K, past nout, and for a null row); loads only
template <int NT, bool KT>
__device__ inline void wide_load(const float* __restrict__ ar, const float* __restrict__ B, int K, int nout, int k0,
                                 float (&a)[4], float (&b)[NT][4]) {
  const int lane = threadIdx.x & 63, j = lane & 15, kk = lane >> 4;
  const int k = k0 + 4 * kk;
  const bool kin = k < K;  // K % 4 == 0: the lane's four k are all inside or all outside
  a[0] = a[1] = a[2] = a[3] = 0.f;
  if (kin && ar != nullptr) {
    const float4 v = *reinterpret_cast<const float4*>(ar + k);
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
  }
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    const int o = 16 * c + j;
    b[c][0] = b[c][1] = b[c][2] = b[c][3] = 0.f;
    if (kin && o < nout) {
      if constexpr (KT) {
        const float4 v = *reinterpret_cast<const float4*>(B + (long long)o * K + k);
        b[c][0] = v.x; b[c][1] = v.y; b[c][2] = v.z; b[c][3] = v.w;
      } else {
        const float* q = B + (long long)k * nout + o;
        b[c][0] = q[0]; b[c][1] = q[nout]; b[c][2] = q[2 * nout]; b[c][3] = q[3 * nout];
      }
    }
  }
}

template <int NT>
__device__ inline void wide_block(const float (&a)[4], const float (&b)[NT][4], f32x4 (&acc)[NT]) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[c][s], acc[c], 0, 0, 0);
}

// The loads run two blocks ahead of the MFMAs (a wave is alone on its rows: without that each block
// waited a full memory round trip); the blocks still enter the chain in ascending k0.
// The chain of wave g of a workgroup: the blocks k0 = 16 (g + WIDE_KS i), i = 0, 1, ... (kb = 16 g, kstep = 16 WIDE_KS).
template <int NT, bool KT>
__device__ inline void wide_dot(const float* __restrict__ ar, const float* __restrict__ B, int K, int nout, int kb,
                                int kstep, f32x4 (&acc)[NT]) {
  float a0[4], a1[4], an0[4], an1[4];
  float b0[NT][4], b1[NT][4], bn0[NT][4], bn1[NT][4];
  wide_load<NT, KT>(ar, B, K, nout, kb, a0, b0);
  wide_load<NT, KT>(ar, B, K, nout, kb + kstep, a1, b1);
  for (int k0 = kb; k0 < K; k0 += 2 * kstep) {
    wide_load<NT, KT>(ar, B, K, nout, k0 + 2 * kstep, an0, bn0);
    wide_load<NT, KT>(ar, B, K, nout, k0 + 3 * kstep, an1, bn1);
    wide_block<NT>(a0, b0, acc);
    if (k0 + kstep < K) wide_block<NT>(a1, b1, acc);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a0[s] = an0[s];
      a1[s] = an1[s];
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        b0[c][s] = bn0[c][s];
        b1[c][s] = bn1[c][s];
      }
    }
  }
}

// the wave's accumulator tiles into a [16][16 NT + 4] LDS image, so[row][output]
template <int NT>
__device__ inline void wide_acc_to_lds(const f32x4 (&acc)[NT], float (*so)[16 * NT + 4]) {
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int v = 0; v < 4; ++v) so[4 * q + v][16 * c + j] = acc[c][v];
}

// ------------------------------------------------------------------ policy head forward
// policy_finish for a wide head: lane j < A owns action dimension j and is handed its own two head
// outputs (mu_raw = out[j], ls_raw = out[A + j], read from the tile's LDS image: no select chain).
// The tail is policy_finish's, statement by statement.
__device__ inline void policy_finish_wide(const PolicyParams& p, int b, int t, float mu_raw, float ls_raw, int lane) {
  const HeadParams& hp = p.head;
  const int A = p.A, hd = hp.hd;
  float term = 0.f;
  const int lj = lane < A ? lane : 0;
  const float bmu = hp.bh[t * hd + lj], bls = hp.bh[t * hd + A + lj];
  const float eps_in = p.eps != nullptr ? p.eps[(long long)b * A + lj] : 0.f;
  if (lane < A) {
    const float mu = mu_raw + bmu;
    const float ls = ls_raw + bls;
    float eps;
    if (p.eps != nullptr) {
      eps = eps_in;
    } else {  // stream ids in use are 1 .. 8: the offsets 16 (lane >> 2) <= 240 collide with none
      float nz[4];
      const uint32_t nrow = p.noise_div > 0 ? (uint32_t)(b / p.noise_div) : (uint32_t)b;
      normal4(p.seed, p.stream_id + 16u * (uint32_t)(lane >> 2), *p.counter, nrow, nz);
      eps = nz[lane & 3];
    }
    const float lsc = fminf(fmaxf(ls, p.ls_min), p.ls_max);
    const float sigma = expf(lsc);
    const float x = mu + sigma * eps;
    const float a = tanhf(x);
    term = -0.5f * eps * eps - HALF_LOG_2PI - logf(sigma) - 2.0f * (LOG2F - x - softplusf(-2.0f * x));
    p.a_out[(long long)b * p.ld_a_out + lane] = a;
    if (p.a_out2) p.a_out2[(long long)b * p.ld_a_out2 + lane] = a;
    if (p.a_planes && p.ap_rec) {
      _Float16 h, l;
      split2h_dev(a, exp2i(p.ap_rec->e), h, l);
      const long long o = (long long)b * p.ap_ld + lane;
      reinterpret_cast<_Float16*>(p.a_planes)[o] = h;
      reinterpret_cast<_Float16*>(p.a_planes)[o + p.ap_ps] = l;
    } else if (p.a_planes) {
      __bf16 h, m, l;
      split3_dev(a, h, m, l);
      const long long o = (long long)b * p.ap_ld + lane;
      p.a_planes[o] = h;
      p.a_planes[o + p.ap_ps] = m;
      p.a_planes[o + 2 * p.ap_ps] = l;
    }
    if (p.cache) {
      float* c = p.cache + (long long)b * 5 * A;
      c[lane] = mu;
      c[A + lane] = ls;
      c[2 * A + lane] = x;
      c[3 * A + lane] = a;
      c[4 * A + lane] = eps;
    }
  }
  term = wsum(term);
  if (lane == 0) p.logpi[b] = term;
}

// one workgroup (WIDE_KS waves), one tile: row_a is the batch row this lane's A row holds (row l & 15 of the
// tile), < 0 none; the first nfin tile rows are finished (16, or 1 when every A row is the same batch row),
// wave g finishing rows g, g + WIDE_KS, ...
template <int NT>
__device__ inline void policy_wide_tile(const PolicyParams& p, int t, int row_a, int nfin,
                                        float (*sp)[16][16 * NT + 4]) {
  const HeadParams& hp = p.head;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  float(*so)[16 * NT + 4] = sp[g];
  const int th = hp.shared ? 0 : t;  // the head's block (a shared head has one)
  const long long woff = (long long)th * hp.W * hp.hd;
  f32x4 acc[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ar = row_a >= 0 ? hp.h + (long long)row_a * hp.W : nullptr;
  if (hp.WhT != nullptr) wide_dot<NT, true>(ar, hp.WhT + woff, hp.W, hp.hd, 16 * g, 16 * WIDE_KS, acc);
  else wide_dot<NT, false>(ar, hp.Wh + woff, hp.W, hp.hd, 16 * g, 16 * WIDE_KS, acc);
  wide_acc_to_lds<NT>(acc, so);
  __syncthreads();
  const int lj = lane < p.A ? lane : 0;
  for (int r = g; r < nfin; r += WIDE_KS) {
    const int b = __shfl(row_a, r);  // lane r holds tile row r's batch row
    if (b < 0) continue;
    const float mu = ((sp[0][r][lj] + sp[1][r][lj]) + sp[2][r][lj]) + sp[3][r][lj];
    const float ls = ((sp[0][r][p.A + lj] + sp[1][r][p.A + lj]) + sp[2][r][p.A + lj]) + sp[3][r][p.A + lj];
    policy_finish_wide(p, b, th, mu, ls, lane);
  }
}

// grouped (task_rows lists) and pair forms: workgroup (task t, 16-row tile of its list, which of the pair)
template <int NT>
__global__ __launch_bounds__(64 * WIDE_KS) void policy_head_wide_kernel(PolicyPair pp) {
  __shared__ float so[WIDE_KS][16][16 * NT + 4];
  const PolicyParams& p = pp.p[blockIdx.z];
  const int t = blockIdx.x;
  const int n = p.counts[t];
  const int j0 = blockIdx.y * 16;
  if (j0 >= n) return;
  const int jj = j0 + (threadIdx.x & 15);
  const int row_a = jj < n ? p.rows[(long long)t * p.max_rows + jj] : -1;
  policy_wide_tile<NT>(p, t, row_a, 16, so);
}

// rollout form (rows without task lists): a workgroup per row, the row in all 16 A rows of its tile (the row's
// chains are the grouped form's: bitwise the same outputs; rollouts hold at most a few dozen rows)
template <int NT>
__global__ __launch_bounds__(64 * WIDE_KS) void policy_head_wide_row_kernel(PolicyParams p) {
  __shared__ float so[WIDE_KS][16][16 * NT + 4];
  const int b = blockIdx.x;
  policy_wide_tile<NT>(p, p.head.task[b], b, 1, so);
}

// ------------------------------------------------------------------ head backward (data)
// Workgroup: 16 columns w0 .. w0 + 15 of (task t, member e); wave rs is row slice rs.  The 16 head rows
// Wh[t][w0 + j][.] are staged in LDS once for the four waves; wave rs then walks the task's 16-row tiles
// rt = rs, rs + HB_RS, ... : g[row][w0 + j] = sum_o dout[row][o] Wh[t][w0 + j][o] as ONE fmaf chain over
// o = 0, 1, ..., hd - 1 in order (hd rounded up to 4 with exact zeros), the ReLU mask from h (each h
// element read once), and the stores of head_bwd_put (fp32 dz and / or the split3 / split2h planes).
// dbp[(t, rs)][w]: per row tile the 16 masked rows are added as a butterfly over the tile row index
// (xor 1, 2, 4, 8; rows past n_t are zeros), then the tiles in ascending rt.
__global__ __launch_bounds__(256) void head_bwd_data_wide_kernel(HeadParams hp, const float* __restrict__ dout,
                                                                  long long s_dout, float* __restrict__ dz,
                                                                  PlaneOut po, float* __restrict__ dbp,
                                                                  const int* __restrict__ counts,
                                                                  const int* __restrict__ rows, int max_rows) {
  __shared__ float sw[16][WIDE_MAX_HD + 4];  // pitch 132: lane (kk, j) reads bank 4 j + kk + o0, all distinct
  __shared__ __attribute__((aligned(16))) float so_all[HB_RS][16][20];  // a wave's tile, [row][column]
  __shared__ float scr[16];
  if (po.p && po.rc) {  // split2h: the planes' exponent, as head_bwd_data_body
    const float md = rec_max(po.rd, po.nd, scr);
    const int ec = plane_exp(po.kmul * md * (po.rw->amax[1] + po.w_add));
    po.w_add = exp2i(ec);
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) po.rc->e = ec;
  }
  const int e = blockIdx.z, t = blockIdx.y, rs = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63, j = lane & 15, kk = lane >> 4;
  const int w0 = blockIdx.x * 16, hd = hp.hd, hd4 = (hd + 3) & ~3;
  const int n = counts[t];
  const int* rl = rows + (long long)t * max_rows;
  float(*so)[20] = so_all[rs];
  {
    const float* Wt = hp.Wh + e * hp.sWh + (long long)(hp.shared ? 0 : t) * hp.W * hd;
    for (int idx = threadIdx.x; idx < 16 * hd4; idx += 256) {
      const int jj = idx / hd4, o = idx - jj * hd4;
      sw[jj][o] = (o < hd && w0 + jj < hp.W) ? Wt[(long long)(w0 + jj) * hd + o] : 0.f;
    }
  }
  __syncthreads();
  const int r = lane >> 2, c4 = 4 * (lane & 3), w = w0 + c4;  // the store layout: tile row r, 4 columns
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int rt0 = 0; rt0 * 16 < n; rt0 += HB_RS) {  // the same trip count in every wave (the barriers below)
    const int rt = rt0 + rs;
    const bool live = rt * 16 < n;  // (wave-uniform)
    int row_a = -1;
    if (live) {
      const int jr = rt * 16 + j;
      row_a = jr < n ? rl[jr] : -1;
      const float* d = row_a >= 0 ? dout + e * s_dout + (long long)row_a * hd : nullptr;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int o0 = 0; o0 < hd4; o0 += 4) {
        const int o = o0 + kk;
        const float a = (d != nullptr && o < hd) ? d[o] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sw[j][o], acc, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) so[4 * kk + v][j] = acc[v];
    }
    __syncthreads();
    if (live) {
      const int b = __shfl(row_a, r);
      float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b >= 0 && w < hp.W) {
        const float4 g = *reinterpret_cast<const float4*>(&so[r][c4]);
        const float4 h = *reinterpret_cast<const float4*>(hp.h + e * hp.sh + (long long)b * hp.W + w);
        out.x = h.x > 0.f ? g.x : 0.f;
        out.y = h.y > 0.f ? g.y : 0.f;
        out.z = h.z > 0.f ? g.z : 0.f;
        out.w = h.w > 0.f ? g.w : 0.f;
        head_bwd_put<1>(hp, e, b, w, out, dz, po);
      }
      float4 ts = out;
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) {  // the lane's bits 2 .. 5 are the tile row
        ts.x += __shfl_xor(ts.x, o);
        ts.y += __shfl_xor(ts.y, o);
        ts.z += __shfl_xor(ts.z, o);
        ts.w += __shfl_xor(ts.w, o);
      }
      cs.x += ts.x; cs.y += ts.y; cs.z += ts.z; cs.w += ts.w;
    }
    __syncthreads();
  }
  if (dbp != nullptr && lane < 4 && w < hp.W)
    *reinterpret_cast<float4*>(dbp + ((long long)e * gridDim.y * HB_RS + t * HB_RS + rs) * hp.W + w) = cs;
}

// ------------------------------------------------------------------ head backward (weights)
// Workgroup (task t, 64 columns, member e), wave g its columns w0 = 64 by + 16 g .. + 15 and ALL outputs
// (NT tiles), so each h element is read once.  dWh[t][w][o] = sum_j h[row_j][w] dout[row_j][o]: ONE fmaf
// chain over the task's row list in list order j = 0, 1, ..., n_t - 1 (rounded up to 4 with exact zeros).
// dbh[t][o] = sum_j dout[row_j][o]: thread o adds the rows in the same order.
template <int NT>
__global__ __launch_bounds__(256) void head_bwd_weight_wide_kernel(HeadParams hp, const float* __restrict__ dout,
                                                                    long long s_dout, const int* __restrict__ counts,
                                                                    const int* __restrict__ rows, int max_rows,
                                                                    float* __restrict__ dWh, float* __restrict__ dbh) {
  const int t = blockIdx.x, e = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kk = lane >> 4;
  const int w0 = blockIdx.y * 64 + 16 * wave, hd = hp.hd;
  const int n = counts[t];
  const int* rl = rows + (long long)t * max_rows;
  const float* h = hp.h + e * hp.sh;
  const float* d = dout + e * s_dout;
  if (w0 < hp.W) {  // (wave-uniform)
    f32x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool win = w0 + j < hp.W;
    for (int k0 = 0; k0 < n; k0 += 16) {  // four k-steps' loads in flight; they enter the chain in order
      int row[4];
      bool rin[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int jr = k0 + 4 * u + kk;
        rin[u] = jr < n;
        row[u] = rl[rin[u] ? jr : n - 1];
      }
      float a[4], b[4][NT];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = (rin[u] && win) ? h[(long long)row[u] * hp.W + w0 + j] : 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c)
          b[u][c] = (rin[u] && 16 * c + j < hd) ? d[(long long)row[u] * hd + 16 * c + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + 4 * u < n) {  // (uniform)
#pragma unroll
          for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u][c], acc[c], 0, 0, 0);
        }
      }
    }
    float* out = dWh + e * hp.sWh + (long long)t * hp.W * hd;
#pragma unroll
    for (int c = 0; c < NT; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int w = w0 + 4 * kk + v, o = 16 * c + j;
        if (w < hp.W && o < hd) out[(long long)w * hd + o] = acc[c][v];
      }
  }
  if (blockIdx.y == 0 && (int)threadIdx.x < hd) {
    float s = 0.f;
    for (int jr = 0; jr < n; ++jr) s += d[(long long)rl[jr] * hd + threadIdx.x];
    dbh[e * hp.sbh + t * hd + threadIdx.x] = s;
  }
}

// The shared head's form (HeadParams::shared, heads.hip head_bwd_weight_shared_kernel): workgroup (row chunk c,
// 64 columns, member e), wave g its 16 columns and all outputs.  The chunk's partial ws_w[e][c][w][o] is ONE
// fmaf chain over the chunk's rows r0, r0 + 1, ... in order (rounded up to 4 with exact zeros); ws_b[e][c][o]:
// thread o adds the chunk's rows of dout in the same order.  head_shared_finish_kernel adds the chunks.
template <int NT>
__global__ __launch_bounds__(256) void head_bwd_weight_shared_wide_kernel(HeadParams hp, const float* __restrict__ dout,
                                                                           long long s_dout, float* __restrict__ ws_w,
                                                                           float* __restrict__ ws_b) {
  const int c0 = blockIdx.x, e = blockIdx.z, chunks = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kk = lane >> 4;
  const int w0 = blockIdx.y * 64 + 16 * wave, hd = hp.hd;
  const int r0 = c0 * HEAD_SHARED_ROWS, r1 = min(r0 + HEAD_SHARED_ROWS, hp.B);
  const float* h = hp.h + e * hp.sh;
  const float* d = dout + e * s_dout;
  if (w0 < hp.W) {  // (wave-uniform)
    f32x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool win = w0 + j < hp.W;
    for (int k0 = r0; k0 < r1; k0 += 16) {  // four k-steps' loads in flight; they enter the chain in order
      float a[4], b[4][NT];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = k0 + 4 * u + kk;
        const bool rin = row < r1;
        a[u] = (rin && win) ? h[(long long)row * hp.W + w0 + j] : 0.f;
#pragma unroll
        for (int c = 0; c < NT; ++c) b[u][c] = (rin && 16 * c + j < hd) ? d[(long long)row * hd + 16 * c + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k0 + 4 * u < r1) {  // (uniform)
#pragma unroll
          for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u][c], acc[c], 0, 0, 0);
        }
      }
    }
    float* out = ws_w + ((long long)e * chunks + c0) * hp.W * hd;
#pragma unroll
    for (int c = 0; c < NT; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int w = w0 + 4 * kk + v, o = 16 * c + j;
        if (w < hp.W && o < hd) out[(long long)w * hd + o] = acc[c][v];
      }
  }
  if (blockIdx.y == 0 && (int)threadIdx.x < hd) {
    float s = 0.f;
    for (int row = r0; row < r1; ++row) s += d[(long long)row * hd + threadIdx.x];
    ws_b[((long long)e * chunks + c0) * hd + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------ action grad
// action_grad_rows' tail for one row, lane j < A owning action dimension j and handed its own ga[b][j]
// (statement by statement; no contraction, as there); returns the lane's max |dout| (0 past A)
__device__ inline float action_grad_tail_wide(const ActionGradParams& p, int b, float ga, int lane) {
#pragma clang fp contract(off)
  const int A = p.A;
  const int lj = lane < A ? lane : 0;
  const float* c = p.cache + (long long)b * 5 * A;
  const float ls = c[A + lj], a = c[3 * A + lj], eps = c[4 * A + lj];
  const float g_logpi = p.alpha_w[b];
  float ex_d = 0.f;
  if (p.a_data != nullptr) {
    if (lane < A) ex_d = p.a_data[(long long)b * p.ld_a_data + lane] - a;
    const float ex = wsum(ex_d * ex_d) / (float)A;
    if (lane == 0) {
      p.row_loss[b] = p.row_loss[b] - ex;
      p.row_explore[b] = ex;
    }
  }
  if (lane >= A) return 0.f;
  float g_a = ga;
  if (p.a_data != nullptr) g_a = g_a + p.explore_scale * ex_d;
  const float sigma = expf(fminf(fmaxf(ls, p.ls_min), p.ls_max));
  const float g_x = g_a * (1.0f - a * a) + g_logpi * 2.0f * a;
  const float g_ls = (g_x * sigma * eps - g_logpi) * clip_grad(ls, p.ls_min, p.ls_max);
  p.dout[(long long)b * 2 * A + lane] = g_x;
  p.dout[(long long)b * 2 * A + A + lane] = g_ls;
  return fmaxf(fabsf(g_x), fabsf(g_ls));
}

// ga[b][j] = sum_e sum_w dz1[e][b][w] W0[e][j][w]: workgroup = 16 consecutive batch rows and ALL A outputs
// (NT tiles), so each dz1 row is read once.  Per output wide_dot's WIDE_KS partial sums, each running on
// through the members (e = 0 in wide_dot's k order, then e = 1 on the same accumulator, ...), then
// ((P0 + P1) + P2) + P3; wave g finishes tile rows g, g + WIDE_KS, ...  A row whose member-e slot is < 0
// (compacted dz1) enters as a row of zeros: fmaf(0, w, acc) = acc, the dense sum.
// Grid-stride over the tiles (at most PLANE_REC_PARTS workgroups: one max |dout| per workgroup).
template <int NT>
__global__ __launch_bounds__(64 * WIDE_KS) void action_grad_wide_kernel(ActionGradParams p) {
  __shared__ float sg[WIDE_KS][16][16 * NT + 4];
  __shared__ float smx[WIDE_KS];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int lj = lane < p.A ? lane : 0;
  float omx = 0.f;
  for (int tile = blockIdx.x; tile * 16 < p.B; tile += gridDim.x) {
    const int b = tile * 16 + (lane & 15);
    f32x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < p.E; ++e) {
      const int sl = b < p.B ? (p.slot ? p.slot[(long long)e * p.B + b] : b) : -1;
      wide_dot<NT, true>(sl >= 0 ? p.dz1 + e * p.s_dz + (long long)sl * p.Wc : nullptr, p.W0 + e * p.s_W0, p.Wc, p.A,
                         16 * g, 16 * WIDE_KS, acc);
    }
    wide_acc_to_lds<NT>(acc, sg[g]);
    __syncthreads();
    for (int r = g; r < 16 && tile * 16 + r < p.B; r += WIDE_KS) {
      const float ga = ((sg[0][r][lj] + sg[1][r][lj]) + sg[2][r][lj]) + sg[3][r][lj];
      omx = fmaxf(omx, action_grad_tail_wide(p, tile * 16 + r, ga, lane));
    }
    __syncthreads();
  }
  if (p.dout_rec) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omx = fmaxf(omx, __shfl_xor(omx, o));
    if (lane == 0) smx[g] = omx;
    __syncthreads();
    if (threadIdx.x == 0) p.dout_rec->amax[blockIdx.x] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

// launches: NT by the output count
#define WIDE_NT_LAUNCH(NTV, K, grid, block, st, ...)                                      \
  switch (NTV) {                                                                          \
    case 1: hipLaunchKernelGGL((K<1>), grid, block, 0, st, __VA_ARGS__); break;           \
    case 2: hipLaunchKernelGGL((K<2>), grid, block, 0, st, __VA_ARGS__); break;           \
    case 4: hipLaunchKernelGGL((K<4>), grid, block, 0, st, __VA_ARGS__); break;           \
    default: hipLaunchKernelGGL((K<8>), grid, block, 0, st, __VA_ARGS__); break;          \
  }
