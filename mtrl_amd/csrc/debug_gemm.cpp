// debug_gemm.cpp -- the test-only entry points of the GEMMs (include/mtsac_debug.h), on debug_harness.h:
// gemm_f32 / gemm_x3, the plane GEMMs gemm_x3p / gemm_x3f / gemm_x3s / gemm_x3f_ragged, their finishing
// passes, and the timing entries.
#include "../../include/mtsac.h"
#include "../../include/mtsac_debug.h"
#include "debug_harness.h"

using namespace mtsac;

namespace {

int fail(int code, const std::string& msg) {
  set_last_error(msg.c_str());
  return code;
}

// the timing entries' operands: uniform in [-1, 1)
__global__ void fill_rand_f32(float* p, long long n, unsigned seed) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned x = (unsigned)i * 2654435761u ^ seed;
  x ^= x >> 13;
  x *= 0x5bd1e995u;
  x ^= x >> 15;
  p[i] = ((float)(x & 0xFFFFFF) / 8388608.0f) - 1.0f;
}
void fill_rand(float* p, long long n, unsigned seed) {
  hipLaunchKernelGGL(fill_rand_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, p, n, seed);
}

void operand_a(SplitGemmParams& g, const PlaneOp& o) {
  g.A = o.p; g.lda = o.ld; g.pA = o.ps; g.sA = o.sb; g.a_kmajor = o.g.kmajor;
}
void operand_b(SplitGemmParams& g, const PlaneOp& o) {
  g.B = o.p; g.ldb = o.ld; g.pB = o.ps; g.sB = o.sb; g.b_kmajor = o.g.kmajor; g.b_frag = o.g.frag;
}
void operand_mask16(SplitGemmParams& g, const PlaneOp& o) {
  g.mask16 = o.p; g.ldm = (int)o.ld; g.sMask = o.sb;
}

// the older entries hand the launcher a zero buffer where the caller passed no bias / mask
const float* in_or_zeros(Guarded& g, const float* host, size_t n) { return host ? g.in(host, n) : g.zeros<float>(n); }

// What mtsac_debug_gemm_x3f_ld adds to mtsac_debug_gemm_x3f: the engine's padded strides of the output and
// mask planes, guarded outputs that start as all-ones, the column-sum partials with their finish, and info.
struct X3fForm {
  bool ld;
  int kpad;          // K padded to 64, or for gemm_x3s in the engine's form to its 32
  int ld_n, rows_p;  // row stride and rows per plane (dense: N, M)
  float *dbp, *db;
  int* info;
};

int run_gemm_x3f(const EpiFlags& f, const X3fForm& o, int batch, int M, int N, int K, const float* A, const float* B,
                 float* C, const float* bias, const float* mask, float* Csum) {
  const int epi = f.epi;
  const size_t nA = (size_t)M * K * batch, nB = (size_t)N * K * batch, nC = (size_t)M * N * batch;
  const size_t nbias = (size_t)N * batch;
  const long long pp = (long long)o.rows_p * o.ld_n;  // plane stride of the output and mask planes
  const int maxrt = gemm_x3f_max_row_tiles(M);
  const bool bias_in_b = epi == EPI_BIAS_RELU && bias;
  Guarded gd;
  // split2h: records of A, B (its max covering the bias, as a trunk record does), the mask and C
  std::vector<PlaneRec> hrec = host_recs({}, 4);
  if (f.h2)
    hrec = host_recs({host_amax(A, nA), std::max(host_amax(B, nB), bias_in_b ? host_amax(bias, nbias) : 0.f),
                      mask ? host_amax(mask, nC) : 1.f},
                     1);
  PlaneRec* rec = gd.in(hrec.data(), 4);
  const float *dA = gd.in(A, nA), *dB = gd.in(B, nB);
  const float* dbias = o.ld ? gd.in(bias, nbias) : in_or_zeros(gd, bias, nbias);
  const float* dmask = o.ld ? gd.in(mask, nC) : in_or_zeros(gd, mask, nC);
  // outputs: all-ones between guard bands, or as the dense entry has them, zeros without bands
  float* dC = f.ponly ? nullptr : o.ld ? gd.out<float>(nC, "C") : gd.zeros<float>(nC);
  __bf16* dCp = o.ld ? gd.out<__bf16>((size_t)3 * pp * batch, "C planes") : gd.zeros<__bf16>((size_t)3 * pp * batch);
  float* d_dbp = o.ld ? gd.out<float>((size_t)batch * maxrt * N, "dbp") : nullptr;
  float* d_db = o.ld ? gd.out<float>(nbias, "db") : nullptr;
  if (!gd.ok) return -12;
  PlaneGeom ga(false, f.h2 ? &rec[0].e : nullptr), gb(false, f.h2 ? &rec[1].e : nullptr),
      gm(false, f.h2 ? &rec[2].e : nullptr);
  ga.kpad = gb.kpad = o.kpad;
  ga.rows_p = gm.rows_p = o.rows_p;  // zero rows past M
  gb.frag = f.bfrag;
  gm.ld = o.ld_n;
  const PlaneOp Ap = plane_alloc(gd.mem, batch, M, K, ga), Bp = plane_alloc(gd.mem, batch, N, K, gb);
  const PlaneOp Mp = f.m16 ? plane_alloc(gd.mem, batch, M, N, gm) : PlaneOp{};
  if (!Ap.p || !Bp.p || (f.m16 && !Mp.p)) return -12;
  SplitGemmParams g{};
  operand_a(g, Ap);
  operand_b(g, Bp);
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.bias = dbias; g.sBias = N;
  g.ldm = N; g.sMask = (long long)M * N;
  if (f.m16) operand_mask16(g, Mp);
  if (!f.m16 || !o.ld) g.mask = dmask;
  g.pMask = o.ld || f.h2 ? pp : 0;
  if (Csum) {
    g.Cp = dCp; g.ldcp = o.ld_n; g.pC = pp; g.sCp = 3 * pp;
  }
  g.M = M; g.N = N; g.K = (int)Ap.ld;
  g.np = f.np();
  int nparts = 0;
  if (o.ld) {
    g.dbp = d_dbp;
    g.nparts = &nparts;
  }
  if (f.h2) {
    g.ra = rec + 0; g.na = 1;
    g.rb = rec + 1; g.nb = 1;
    g.rc = rec + 3;
    g.bias_in_b = bias_in_b ? 1 : 0;
    g.kmul = (float)K;
  }
  if (f.autosplit) {
    g.ws = gd.zeros<float>((size_t)std::max(gemm_x3f_ws_floats(M, N, g.K, batch), 1LL));
    g.splits = -1;
    if (f.fin) g.cnt = gd.zeros<int>((size_t)GEMM_X3F_CNT);
    if (!gd.ok) return -12;
  }
  if (f.small ? !gemm_x3s_ok(g, epi, batch) : !gemm_x3f_ok(g, epi, batch)) return -95;
  // rows per column-sum chunk and the chunk count, by the rule the engine's dgrad_params uses
  int bm = 0, chunks = 0;
  if (o.ld) {
    bm = dbp_chunk_rows(g, epi, batch, !f.small);
    chunks = (M + bm - 1) / bm;
    if (chunks > maxrt) return -95;
  }
  // -22 and -95 are behind: the first launches
  plane_split(Ap, dA, (long long)M * K);
  plane_split(Bp, dB, (long long)N * K);
  if (f.m16) plane_split(Mp, dmask, (long long)M * N);
  int rc = 0;
  if (o.ld && (rc = sync_rc("split_planes"))) return rc;
  int slices = 1;
  if (f.small) gemm_x3s(g, epi, batch, nullptr);
  else slices = gemm_x3f(g, epi, batch, nullptr);
  if (o.ld) {
    colsum_finish(d_dbp, N, chunks, batch, d_db, N, nullptr);
  } else if (const hipError_t le = hipGetLastError()) {  // a launch the runtime refused leaves C as it was
    fprintf(stderr, "[mtsac_debug_gemm_x3f] launch refused: %s\n", hipGetErrorString(le));
    return -6;
  }
  if ((rc = sync_rc(f.small ? "gemm_x3s" : "gemm_x3f")) || (o.ld && (rc = gd.check()))) return rc;
  int ec = 0;
  if (f.h2 && !gd.back(&ec, &rec[3].e, 1)) return -5;
  if (dC && !gd.back(C, dC, nC)) return -5;
  // bf16 keeps the high plane only: gemm_x3f leaves the other two alone (all-ones when guarded, else zeros,
  // which the dense entry has always added)
  for (int z = 0; Csum && z < batch; ++z)
    if (!planes_sum(dCp + (size_t)z * 3 * pp, (size_t)3 * pp, (size_t)pp, (size_t)pp, f.h2, ec, Csum + (size_t)z * pp,
                    o.ld && f.np() == 1))
      return -5;
  if (!o.ld) return 0;
  // split launches: the in-launch finish keeps the split row tile, the finishing pass sums shorter chunks
  int* info = o.info;
  info[0] = f.small ? 3 : slices <= 1 ? 0 : bm == gemm_x3f_split_bm(M, N, g.K, batch) ? 1 : 2;
  info[1] = bm;
  info[2] = chunks;
  info[3] = slices;
  info[4] = nparts;
  info[5] = maxrt;
  info[6] = ec;
  info[7] = f.small ? gemm_x3s_ti(M, N, batch) : slices > 1 ? gemm_x3f_split_bm(M, N, g.K, batch) : gemm_x3f_bm(g, batch);
  return gd.back(o.dbp, d_dbp, (size_t)batch * maxrt * N) && gd.back(o.db, d_db, nbias) ? 0 : -5;
}

// gemm_f32 / gemm_x3 of the timing and the checking entry
void launch_gemm(int precision, const GemmParams& g, int kind, int epi, int batch) {
  if (precision == MTSAC_FP32_SPLIT3)
    gemm_x3(g, (GemmKind)kind, epi, batch, nullptr);
  else
    gemm_f32(g, (GemmKind)kind, epi, batch, nullptr);
}

}  // namespace

extern "C" {

int mtsac_debug_gemm(int precision, int kind, int epi, int batch, int M, int N, int K, const float* A, int lda, int a_shared,
                     const float* B, int ldb, float* C, int ldc, const float* bias, const float* mask, int ldm,
                     float* db) {
  const int splits = (precision >> 8) & 255;
  precision &= 255;
  // null A / B / C: Guarded::in would hand the kernel a null operand
  if (kind < 0 || kind > 2 || batch < 1 || M < 1 || N < 1 || K < 1 || !A || !B || !C)
    return fail(-22, "bad gemm arguments");
  const bool ta = kind == 2, tb = kind == 1;
  const long long a_rows = ta ? K : M, b_rows = tb ? N : K;
  const long long sA = a_rows * lda, sB = b_rows * ldb, sC = (long long)M * ldc;
  Guarded gd;
  GemmParams g{};
  g.A = gd.in(A, (size_t)(a_shared ? sA : sA * batch)); g.lda = lda; g.sA = a_shared ? 0 : sA;
  g.B = gd.in(B, (size_t)sB * batch); g.ldb = ldb; g.sB = sB;
  g.C = gd.in(C, (size_t)sC * batch); g.ldc = ldc; g.sC = sC;  // the caller's C: elements outside [M][N] survive
  g.bias = gd.in(bias, (size_t)N * batch); g.sBias = N;
  g.mask = gd.in(mask, (size_t)M * ldm * batch); g.ldm = ldm; g.sMask = (long long)M * ldm;
  g.db = db ? gd.zeros<float>((size_t)N * batch) : nullptr; g.sDb = N;
  g.M = M; g.N = N; g.K = K;
  g.splits = splits;
  g.ws = splits > 1 ? gd.zeros<float>((size_t)gemm_ws_floats(M, N, batch, splits)) : nullptr;
  if (!gd.ok) return fail(-12, "hipMalloc failed");
  launch_gemm(precision, g, kind, epi, batch);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(C, g.C, sizeof(float) * sC * batch, hipMemcpyDeviceToHost);
  if (e == hipSuccess && db) e = hipMemcpy(db, g.db, sizeof(float) * N * batch, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(-5, std::string("debug gemm: ") + hipGetErrorString(e));
  return 0;
}

int mtsac_debug_gemm_bench(int precision, int kind, int epi, int batch, int M, int N, int K, int iters,
                           double* ms_per_launch) {
  const int splits = (precision >> 8) & 255;
  precision &= 255;
  if (kind < 0 || kind > 2 || batch < 1 || M < 1 || N < 1 || K < 1 || iters < 1 || !ms_per_launch)
    return fail(-22, "bad gemm bench arguments");
  const bool ta = kind == 2, tb = kind == 1;
  const int lda = ta ? M : K, ldb = tb ? K : N;
  const long long sA = (long long)(ta ? K : M) * lda, sB = (long long)(tb ? N : K) * ldb, sC = (long long)M * N;
  Guarded gd;
  float *A = gd.zeros<float>((size_t)sA * batch), *B = gd.zeros<float>((size_t)sB * batch);
  float *C = gd.zeros<float>((size_t)sC * batch), *bias = gd.zeros<float>((size_t)N * batch);
  GemmParams g{};
  g.A = A; g.lda = lda; g.sA = sA;
  g.B = B; g.ldb = ldb; g.sB = sB;
  g.C = C; g.ldc = N; g.sC = sC;
  g.bias = bias; g.sBias = N;
  g.mask = C; g.ldm = N; g.sMask = sC;  // any sign pattern will do
  g.db = kind == 2 ? gd.zeros<float>((size_t)N * batch) : nullptr; g.sDb = N;
  g.M = M; g.N = N; g.K = K;
  g.splits = splits;
  g.ws = splits > 1 ? gd.zeros<float>((size_t)gemm_ws_floats(M, N, batch, splits)) : nullptr;
  if (!gd.ok) return fail(-5, "debug gemm bench: hipMalloc failed");
  fill_rand(A, sA * batch, 17u);
  fill_rand(B, sB * batch, 17u);
  fill_rand(C, sC * batch, 17u);
  fill_rand(bias, (long long)N * batch, 17u);
  const hipError_t e = time_launches(iters, [&]() { launch_gemm(precision, g, kind, epi, batch); }, ms_per_launch);
  if (e != hipSuccess) return fail(-5, std::string("debug gemm bench: ") + hipGetErrorString(e));
  return 0;
}

int mtsac_debug_gemm_x3p(int epi, int M, int N, int K, const float* A, int a_kmajor, const float* B, int b_kmajor,
                         float* C, const float* bias, const float* mask, float* Csum) {
  const int splits = (epi >> 8) & 255;
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || !A || !B || !C) return -22;
  const size_t nC = (size_t)M * N;
  Guarded gd;
  const float *dA = gd.in(A, (size_t)M * K), *dB = gd.in(B, (size_t)N * K);
  float* dC = gd.zeros<float>(nC);
  __bf16* dCp = gd.zeros<__bf16>(3 * nC);
  SplitGemmParams g{};
  g.bias = in_or_zeros(gd, bias, (size_t)N);
  g.mask = in_or_zeros(gd, mask, nC); g.ldm = N;
  g.ws = gd.zeros<float>(splits > 1 ? (size_t)gemm_ws_floats(M, N, 1, splits) : 1);
  if (!gd.ok) return -12;
  const PlaneOp Ap = plane_operand(gd.mem, dA, 0, 1, M, K, PlaneGeom(a_kmajor != 0));
  const PlaneOp Bp = plane_operand(gd.mem, dB, 0, 1, N, K, PlaneGeom(b_kmajor != 0));
  if (!Ap.p || !Bp.p) return -12;
  operand_a(g, Ap);
  operand_b(g, Bp);
  g.sA = g.sB = 0;  // one batch entry
  g.C = dC; g.ldc = N;
  if (Csum) {
    g.Cp = dCp; g.ldcp = N; g.pC = (long long)nC;
  }
  g.M = M; g.N = N; g.K = (int)up32(K);
  g.splits = splits;
  gemm_x3p(g, epi, 1, nullptr);
  if (hipDeviceSynchronize() != hipSuccess || !gd.back(C, dC, nC)) return -5;
  return !Csum || planes_sum(dCp, 3 * nC, nC, nC, false, 0, Csum) ? 0 : -5;
}

// the split2h k-major x k-major weight grad alone (mtsac_debug.h)
int mtsac_debug_gemm_x3p_kmajor(int E, int M, int N, int K, int slices, const float* A, const float* B, float* C) {
  if (E < 1 || E > 8 || M < 1 || N < 1 || K < 1 || slices < 1 || slices > 64 || slices > (int)(up32(K) / 32) || !A ||
      !B || !C || (long long)E * K * std::max(M, N) >= (1LL << 28))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t nA = (size_t)E * K * M, nB = (size_t)E * K * N, nC = (size_t)E * M * N;
  Guarded gd;
  // the operands' records as a producer leaves them: max |x| and the plane exponent of that bound
  const std::vector<PlaneRec> hrec = host_recs({host_amax(A, nA), host_amax(B, nB)});
  const PlaneRec* rec = gd.in(hrec.data(), 2);
  const float *dA = gd.in(A, nA), *dB = gd.in(B, nB);
  float* dC = gd.out<float>(nC, "C");  // starts as NaN between two guard bands
  SplitGemmParams g{};
  g.ws = gd.zeros<float>((size_t)std::max(gemm_ws_floats(M, N, E, std::max(slices, 2)), 1LL));
  if (!gd.ok) return -12;
  const PlaneOp Ap = plane_operand(gd.mem, dA, (long long)K * M, E, M, K, PlaneGeom(true, &rec[0].e));
  const PlaneOp Bp = plane_operand(gd.mem, dB, (long long)K * N, E, N, K, PlaneGeom(true, &rec[1].e));
  if (!Ap.p || !Bp.p) return -12;
  operand_a(g, Ap);
  operand_b(g, Bp);
  g.np = 2;
  g.ra = rec; g.na = 1; g.rb = rec + 1; g.nb = 1;
  g.kmul = (float)K;
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.M = M; g.N = N; g.K = (int)up32(K);
  g.splits = slices;
  gemm_x3p(g, EPI_STORE, E, nullptr);
  int rc = 0;
  if ((rc = sync_rc("gemm_x3p k-major")) || (rc = gd.check())) return rc;
  return gd.back(C, dC, nC) ? 0 : -5;
}

int mtsac_debug_gemm_x3p_bench(int epi, int batch, int M, int N, int K, int iters, double* ms_per_launch) {
  const int layout = (epi >> 8) & 3;     // bit 0: A k-major, bit 1: B k-major
  const int splits = (epi >> 16) & 255;  // split-K slices (0/1: none; EPI_STORE: + splitk_reduce; 255: auto)
  const bool fin = (epi >> 12) & 1;      // arrival counters: the weight grads' in-launch reduce
  const bool h2 = (epi >> 13) & 1;       // precision split2h (zero exponents: operands in [-1, 1])
  const bool pout = (epi >> 14) & 1;     // planes out only (the forward's: bias+ReLU planes out)
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || iters < 1 || !ms_per_launch) return -22;
  const long long mn = (long long)M * N;
  Guarded gd;
  PlaneRec* rec = h2 ? gd.zeros<PlaneRec>(3) : nullptr;
  float *fa = gd.zeros<float>((size_t)M * K), *fb = gd.zeros<float>((size_t)N * K);
  float *C = gd.zeros<float>((size_t)mn * batch), *bias = gd.zeros<float>((size_t)N * batch);
  if (!gd.ok) return -12;
  fill_rand(fa, (long long)M * K, 3u);
  fill_rand(fb, (long long)N * K, 5u);
  // one plane set per batch entry (distinct memory, same values)
  const PlaneOp Ap = plane_operand(gd.mem, fa, 0, batch, M, K, PlaneGeom(layout & 1, h2 ? &rec[0].e : nullptr));
  const PlaneOp Bp = plane_operand(gd.mem, fb, 0, batch, N, K, PlaneGeom(layout & 2, h2 ? &rec[1].e : nullptr));
  if (!Ap.p || !Bp.p) return -12;
  SplitGemmParams g{};
  operand_a(g, Ap);
  operand_b(g, Bp);
  if (h2) {
    g.np = 2;
    g.ra = rec; g.rb = rec + 1; g.rc = rec + 2;
    g.kmul = (float)K;
  }
  if (pout) {
    g.Cp = gd.zeros<__bf16>((size_t)3 * mn * batch); g.ldcp = N; g.pC = mn; g.sCp = 3 * mn;
  }
  g.C = pout ? nullptr : C; g.ldc = N; g.sC = mn;
  g.bias = bias; g.sBias = N;
  g.mask = C; g.ldm = N; g.sMask = mn;
  g.M = M; g.N = N; g.K = (int)up32(K);
  if (splits > 1) {
    g.splits = splits == 255 ? -1 : splits;
    const int sw = splits == 255 ? gemm_x3p_splits(M, N, g.K, batch, layout == 3) : splits;
    g.ws = gd.zeros<float>((size_t)mn * batch * std::max(sw, 1));
    if (fin) g.cnt = gd.zeros<int>((size_t)GEMM_X3F_CNT);
  }
  if (!gd.ok) return -12;
  return time_launches(iters, [&]() { gemm_x3p(g, epi, batch, nullptr); }, ms_per_launch) == hipSuccess ? 0 : -5;
}

// gemm_x3f (row-major x row-major planes, K % 64 == 0): C[M][N] = A[M][K] . B[N][K]^T from host
// fp32 arrays, epi 1 bias+ReLU / 2 ReLU mask (fp32 mask, or with bit 8 of epi its bf16 high
// plane); Csum (nullable) receives the sum of the written planes.  -95 when gemm_x3f does not take
// the shape (too few tiles, layout).
int mtsac_debug_gemm_x3f(int epi, int batch, int M, int N, int K, const float* A, const float* B, float* C,
                         const float* bias, const float* mask, float* Csum) {
  const EpiFlags f(epi & 0x7fff);  // this entry has no planes-only form
  if (M < 1 || N < 1 || K < 1 || batch < 1 || !A || !B || !C) return -22;
  if (f.bfrag && N % 16 != 0) return -22;
  return run_gemm_x3f(f, X3fForm{false, 64, N, M, nullptr, nullptr, nullptr}, batch, M, N, K, A, B, C, bias, mask, Csum);
}

// gemm_x3f / gemm_x3s as the engine's trunk calls them (mtsac_debug.h): padded plane strides, guarded
// outputs, the bias grad's column-sum partials and their finish over the engine's own chunk count
int mtsac_debug_gemm_x3f_ld(int epi, int batch, int M, int N, int K, int ld_n, int rows_p, const float* A,
                            const float* B, float* C, const float* bias, const float* mask, float* Csum, float* dbp,
                            float* db, int* info) {
  const EpiFlags f(epi);
  if (M < 1 || N < 1 || K < 1 || batch < 1 || batch > 8 || ld_n < N || ld_n % 4 != 0 || rows_p < M || !A || !B ||
      !Csum || !dbp || !db || !info || (!f.ponly && !C) || (f.epi != EPI_BIAS_RELU && f.epi != EPI_RELU_MASK) ||
      (f.epi == EPI_BIAS_RELU && !bias) || (f.epi == EPI_RELU_MASK && !mask) || (f.bfrag && N % 16 != 0) ||
      (f.h2 && f.bf16) || (long long)batch * rows_p * ld_n >= (1LL << 28))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  return run_gemm_x3f(f, X3fForm{true, f.small ? 32 : 64, ld_n, rows_p, dbp, db, info}, batch, M, N, K, A, B, C, bias, mask, Csum);
}

// The ragged split2h data grad (gemm_x3f_ragged) beside the dense launch it replaces, on host arrays, E = 2:
// A [2][B][K] (dz), W [2][N][K], mask [2][B][N] (the activation), active [2][B] bytes.  The dense launch runs
// on A with the inactive rows zeroed; the ragged one on A's active rows compacted in ascending row order
// (lists from active_rows on dq = active ? -1 : 0), both at the same plane exponents, whatever the tile
// count (the engine's >= 192-workgroup policy is not asked).  flags bit 0: planes out (else fp32), bit 1:
// W planes in the fragment layout (N % 16 == 0).  dense_out / rag_out: fp32 [2][B][N], or the two fp16
// planes as 16-bit words [2][2][B][N]; the ragged buffer and its record's partial maxima start as 0xFF
// bytes / 1e30.  rows_out [2][B]: the lists (0xFF words past n_e).  info [6]: the dense and ragged output
// exponents, the max over the partial maxima of each (float bits), n_0, n_1.
int mtsac_debug_gemm_x3f_ragged(int flags, int B, int N, int K, const float* A, const float* W, const float* mask,
                                const unsigned char* active, void* dense_out, void* rag_out, int* rows_out,
                                int* info) {
  const bool pout = flags & 1, bfrag = (flags >> 1) & 1;
  if (B < 1 || N < 8 || N % 8 != 0 || K < 1 || !A || !W || !mask || !active || !dense_out || !rag_out || !rows_out ||
      !info || (bfrag && N % 16 != 0))
    return -22;
  const int E = 2;
  const size_t nA = (size_t)E * B * K, nW = (size_t)E * N * K, nC = (size_t)E * B * N;
  // host: dq, A with the inactive rows zeroed
  std::vector<float> dq((size_t)E * B), Az(A, A + nA);
  for (int e = 0; e < E; ++e)
    for (int b = 0; b < B; ++b) {
      const bool on = active[(size_t)e * B + b] != 0;
      dq[(size_t)e * B + b] = on ? -1.f : 0.f;
      if (!on) std::fill(Az.begin() + ((size_t)e * B + b) * K, Az.begin() + ((size_t)e * B + b + 1) * K, 0.f);
    }
  Guarded gd;
  float* d_dq = gd.in(dq.data(), dq.size());
  float* dAz = gd.in(Az.data(), nA);
  float* dW = gd.in(W, nW);
  float* dmask = gd.in(mask, nC);
  int* d_n = gd.out<int>(E, "n");
  int* d_rows = gd.out<int>((size_t)E * B, "rows");
  int* d_slot = gd.out<int>((size_t)E * B, "slot");
  if (!gd.ok) return -12;
  active_rows(d_dq, E, B, d_n, d_rows, d_slot, nullptr);
  if (int rc = sync_rc("active_rows")) return rc;
  std::vector<int> hn(E), hrows((size_t)E * B);
  if (!gd.back(hn.data(), d_n, E) || !gd.back(hrows.data(), d_rows, hrows.size())) return -5;
  for (int e = 0; e < E; ++e)
    if (hn[e] < 0 || hn[e] > B) return -5;
  std::vector<float> Ac(nA, 0.f);  // compacted (rows past n_e: zeros, never read)
  for (int e = 0; e < E; ++e)
    for (int s2 = 0; s2 < hn[e]; ++s2) {
      const int b = hrows[(size_t)e * B + s2];
      if (b < 0 || b >= B) return -5;
      std::copy(Az.begin() + ((size_t)e * B + b) * K, Az.begin() + ((size_t)e * B + b + 1) * K,
                Ac.begin() + ((size_t)e * B + s2) * K);
    }
  float* dAc = gd.in(Ac.data(), nA);
  // records: A, W, mask, then the dense and the ragged output's, poisoned so that a stale slot shows
  std::vector<PlaneRec> hrec =
      host_recs({host_amax(Az.data(), nA), host_amax(W, nW), host_amax(mask, nC)}, 2, 0x7fffffff, 1e30f);
  PlaneRec* rec = gd.in(hrec.data(), hrec.size());
  const size_t out_bytes = pout ? nC * 2 * sizeof(__bf16) : nC * sizeof(float);
  unsigned char* dden = gd.out<unsigned char>(out_bytes, "dense out");
  unsigned char* drag = gd.out<unsigned char>(out_bytes, "ragged out");
  if (!gd.ok) return -12;
  PlaneGeom ga(false, &rec[0].e), gw(false, &rec[1].e), gm(false, &rec[2].e);
  ga.kpad = gw.kpad = 64;
  gw.frag = bfrag;
  gm.ld = N;
  const PlaneOp Azp = plane_operand(gd.mem, dAz, (long long)B * K, E, B, K, ga);
  const PlaneOp Acp = plane_operand(gd.mem, dAc, (long long)B * K, E, B, K, ga);
  const PlaneOp Wp = plane_operand(gd.mem, dW, (long long)N * K, E, N, K, gw);
  const PlaneOp Mp = plane_operand(gd.mem, dmask, (long long)B * N, E, B, N, gm);
  if (!Azp.p || !Acp.p || !Wp.p || !Mp.p) return -12;
  SplitGemmParams g{};
  g.np = 2;
  operand_b(g, Wp);
  operand_mask16(g, Mp);
  g.pMask = Mp.ps;
  g.M = B; g.N = N; g.K = (int)Wp.ld;
  g.ra = rec + 0; g.na = 1;
  g.rb = rec + 1; g.nb = 1;
  g.kmul = (float)K;
  int nparts[2] = {0, 0};
  auto outs = [&](unsigned char* o, PlaneRec* rc, int* np_) {
    g.C = nullptr; g.Cp = nullptr; g.rc = nullptr;
    if (pout) {
      g.Cp = reinterpret_cast<__bf16*>(o); g.ldcp = N; g.pC = (long long)B * N; g.sCp = 2 * g.pC;
      g.rc = rc;
    } else {
      g.C = reinterpret_cast<float*>(o); g.ldc = N; g.sC = (long long)B * N;
    }
    g.nparts = np_;
  };
  operand_a(g, Azp);
  outs(dden, rec + 3, &nparts[0]);
  gemm_x3f(g, EPI_RELU_MASK, E, nullptr);  // no workspace: the plain unsplit launch
  if (int rc = sync_rc("dense gemm_x3f")) return rc;
  operand_a(g, Acp);
  outs(drag, rec + 4, &nparts[1]);
  g.rag_n = d_n; g.rag_rows = d_rows; g.rag_ld = B;
  gemm_x3f_ragged(g, nullptr);
  if (int rc = sync_rc("gemm_x3f_ragged")) return rc;
  if (int rc = gd.check()) return rc;
  if (!gd.back(reinterpret_cast<unsigned char*>(dense_out), dden, out_bytes) ||
      !gd.back(reinterpret_cast<unsigned char*>(rag_out), drag, out_bytes) ||
      !gd.back(hrec.data(), rec, hrec.size()))
    return -5;
  std::copy(hrows.begin(), hrows.end(), rows_out);
  for (int k = 0; k < 2; ++k) {
    float m = 0.f;
    for (int i = 0; i < nparts[k] && i < PLANE_REC_PARTS; ++i) m = std::max(m, hrec[3 + k].amax[i]);
    info[k] = hrec[3 + k].e;
    std::memcpy(&info[2 + k], &m, sizeof(float));
  }
  info[4] = hn[0];
  info[5] = hn[1];
  return 0;
}

// time iters launches of the forward-shaped plane GEMM (C = relu(A . B^T + bias) with planes out)
// on device-resident random planes; which: 0 = gemm_x3p (row-major A, k-major B: the engine's
// current forward), 1 = gemm_x3f (row-major both)
int mtsac_debug_gemm_fwd_bench(int which, int epi, int batch, int M, int N, int K, int iters, double* ms_per_launch) {
  const int outs = (epi >> 8) & 3;  // here bits 8-9 are: 0 fp32 + planes, 1 planes only, 2 fp32 only
  const EpiFlags f(epi);            // split2h at zero exponents: the random operands lie in [-1, 1]
  epi = f.epi;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || iters < 1 || !ms_per_launch) return -22;
  const int Kp = (K + 63) / 64 * 64;
  const long long mn = (long long)M * N;
  Guarded gd;
  PlaneRec* rec = gd.zeros<PlaneRec>(3);
  float *fa = gd.zeros<float>((size_t)M * Kp), *fb = gd.zeros<float>((size_t)N * Kp);
  float *C = gd.zeros<float>((size_t)mn * batch), *bias = gd.zeros<float>((size_t)N * batch);
  __bf16* Cp = gd.zeros<__bf16>((size_t)3 * mn * batch);
  if (!gd.ok) return -12;
  fill_rand(fa, (long long)M * Kp, 3u);
  fill_rand(fb, (long long)N * Kp, 5u);
  PlaneGeom gb(which == 0, f.h2 ? &rec[1].e : nullptr);  // gemm_x3p forward: B k-major [K][N]
  gb.frag = f.bfrag && !gb.kmajor;
  const PlaneOp Ap = plane_operand(gd.mem, fa, 0, batch, M, Kp, PlaneGeom(false, f.h2 ? &rec[0].e : nullptr));
  const PlaneOp Bp = plane_operand(gd.mem, fb, 0, batch, N, Kp, gb);
  if (!Ap.p || !Bp.p) return -12;
  SplitGemmParams g{};
  operand_a(g, Ap);
  operand_b(g, Bp);
  if (f.h2) {
    g.ra = rec; g.rb = rec + 1; g.rc = rec + 2;
    g.kmul = (float)K;
    g.pMask = mn;
  }
  g.C = outs == 1 ? nullptr : C; g.ldc = N; g.sC = mn;
  g.bias = bias; g.sBias = N;
  g.mask = C; g.ldm = N; g.sMask = mn;
  g.Cp = outs == 2 ? nullptr : Cp; g.ldcp = N; g.pC = mn; g.sCp = 3 * mn;
  g.M = M; g.N = N; g.K = Kp;
  g.splits = 1;
  g.np = f.np();
  if (f.autosplit) {
    const long long wsf = std::max(gemm_x3f_ws_floats(M, N, Kp, batch), gemm_x3p_ws_floats(M, N, Kp, batch, false));
    g.ws = gd.zeros<float>((size_t)std::max(wsf, 1LL));
    g.splits = -1;
    if (f.fin) g.cnt = gd.zeros<int>((size_t)GEMM_X3F_CNT);
    if (!gd.ok) return -12;
  }
  if (which >= 1 && !gemm_x3f_ok(g, epi, batch)) return -95;
  if (which < 0 && !gemm_x3s_ok(g, epi, batch)) return -95;
  auto run = [&]() {
    if (which == -1) gemm_x3s(g, epi, batch, nullptr);
    else if (which < -1) gemm_x3s_ablate(g, -1 - which, batch, nullptr);  // -2 no loads, -3 no MFMAs
    else if (which >= 2) gemm_x3f_ablate(g, which - 2, batch, nullptr);  // 2 + ablation bits (planes out)
    else if (which == 1) gemm_x3f(g, epi, batch, nullptr);
    else gemm_x3p(g, epi, batch, nullptr);
  };
  return time_launches(iters, run, ms_per_launch) == hipSuccess ? 0 : -5;
}

// the k-major x k-major gemm_x3p weight grad with the bias grad finished from column-sum partials
// (mtsac_debug.h): at once, or through a FinishSink between two unrelated colsum jobs
int mtsac_debug_wgrad_finish(int mode, int E, int M, int N, int K, int chunks, int splits, const float* A,
                             const float* B, const float* part, const int* nb, const float* part_pre,
                             const float* part_post, float* C, float* db, float* db_pre, float* db_post, int* info) {
  if (mode < 0 || mode > 1 || E < 1 || E > 8 || M < 1 || N < 1 || K < 1 || chunks < 1 || splits < 0 || splits > 64 ||
      !A || !B || !part || !C || !db || !info || (long long)E * K * std::max(M, N) >= (1LL << 28))
    return -22;
  if (mode == 1 && (!nb || !part_pre || !part_post || !db_pre || !db_post || nb[0] < 1 || nb[1] < 1 || nb[2] < 1 ||
                    nb[3] < 1))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const int Kp = (int)up32(K);
  Guarded gd;
  const float *dA = gd.in(A, (size_t)E * K * M), *dB = gd.in(B, (size_t)E * K * N);
  const float* dpart = gd.in(part, (size_t)E * chunks * N);
  float* dC = gd.out<float>((size_t)E * M * N, "C");
  float* d_db = gd.out<float>((size_t)E * N, "db");
  const int want = splits == 0 ? gemm_x3p_splits(M, N, Kp, E, true, 3) : splits;
  float* ws = gd.zeros<float>((size_t)std::max(gemm_ws_floats(M, N, E, std::max(want, 2)), 1LL));
  const float *dpre = nullptr, *dpost = nullptr;
  float *d_dbpre = nullptr, *d_dbpost = nullptr;
  if (mode == 1) {
    dpre = gd.in(part_pre, (size_t)E * nb[0] * nb[1]);
    dpost = gd.in(part_post, (size_t)E * nb[2] * nb[3]);
    d_dbpre = gd.out<float>((size_t)E * nb[1], "db_pre");
    d_dbpost = gd.out<float>((size_t)E * nb[3], "db_post");
  }
  if (!gd.ok) return -12;
  const PlaneOp Ap = plane_operand(gd.mem, dA, (long long)K * M, E, M, K, PlaneGeom(true));
  const PlaneOp Bp = plane_operand(gd.mem, dB, (long long)K * N, E, N, K, PlaneGeom(true));
  if (!Ap.p || !Bp.p) return -12;
  SplitGemmParams g{};
  operand_a(g, Ap);
  operand_b(g, Bp);
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.M = M; g.N = N; g.K = Kp;
  g.splits = splits == 0 ? -1 : splits;
  g.ws = ws;
  g.cs_part = dpart; g.cs_chunks = chunks; g.cs_db = d_db; g.cs_sdb = N;
  // the slices gemm_x3p makes of that request (whole 32-deep K tiles per slice)
  int S = 1;
  if (want > 1) {
    const int kchunk = (Kp / 32 + want - 1) / want * 32;
    S = (Kp + kchunk - 1) / kchunk;
  }
  FinishSink sink;
  int this_job = -1;
  if (mode == 1) {
    sink.job[sink.n++] = colsum_job(dpre, nb[1], nb[0], d_dbpre, nb[1]);
    g.defer = &sink;
    this_job = sink.n;
  }
  gemm_x3p(g, EPI_STORE, E, nullptr);
  info[0] = S;
  info[1] = mode == 1 ? 2 : S > 1 ? 1 : 0;  // who finishes the bias grad: colsum_finish, the reduce launch, finish_many
  info[2] = mode == 1 ? sink.n : 0;
  info[3] = mode == 1 && sink.n > this_job ? sink.job[this_job].nred : 0;
  if (mode == 1) {
    if (sink.n != this_job + 1) return -5;  // the launcher did not defer its finish
    sink.job[sink.n++] = colsum_job(dpost, nb[3], nb[2], d_dbpost, nb[3]);
    info[2] = sink.n;
    finish_many(sink, E, nullptr);
  }
  int rc = 0;
  if ((rc = sync_rc("wgrad finish")) || (rc = gd.check())) return rc;
  if (mode == 1 && (!gd.back(db_pre, d_dbpre, (size_t)E * nb[1]) || !gd.back(db_post, d_dbpost, (size_t)E * nb[3])))
    return -5;
  return gd.back(C, dC, (size_t)E * M * N) && gd.back(db, d_db, (size_t)E * N) ? 0 : -5;
}

int mtsac_debug_x3p_geo(int geo) {
  const int old = g_x3p_geo;
  if (geo < 0) {  // restore the default (e.g. the value this function returned)
    g_x3p_geo = -1;
    g_x3p_dbg = g_x3_dbg = 0;
    return old;
  }
  const int g = geo & 255;
  g_x3p_geo = g <= 5 ? g : -1;
  g_x3p_dbg = (geo >> 8) & 255;
  g_x3_dbg = (geo >> 16) & 255;
  return old;
}

int mtsac_debug_x3s_ti(int M, int N, int batch) { return gemm_x3s_ti(M, N, batch); }

}  // extern "C"
