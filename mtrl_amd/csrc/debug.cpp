// debug.cpp -- test-only entry points (include/mtsac_debug.h): the plane GEMMs, the DrQ kernels, the SAC heads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/mtsac.h"
#include "../../include/mtsac_debug.h"
#include "drq_kernels.h"
#include "kernels.h"

using namespace mtsac;

namespace {

long long up32(long long x) { return (x + 31) / 32 * 32; }

__global__ void fill_rand_f32(float* p, long long n, unsigned seed) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned x = (unsigned)i * 2654435761u ^ seed;
  x ^= x >> 13;
  x *= 0x5bd1e995u;
  x ^= x >> 15;
  p[i] = ((float)(x & 0xFFFFFF) / 8388608.0f) - 1.0f;
}

struct DevBuf {
  std::vector<void*> ptrs;
  ~DevBuf() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* get(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
    (void)hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T));
    ptrs.push_back(p);
    return reinterpret_cast<T*>(p);
  }
};

long long up8(long long x) { return (x + 7) / 8 * 8; }

// planes of a fp32 operand stored [rows][K] (k contiguous) or, kmajor, [K][rows]; split in its
// stored orientation: row-major planes [3][rows][up32(K)], k-major planes [3][up32(K)][up8(rows)]
// (zeros in the padding)
void plane_geom(int rows, int K, bool kmajor, long long& ld, long long& ps) {
  ld = kmajor ? up8(rows) : up32(K);
  ps = (kmajor ? up32(K) : (long long)rows) * ld;
}

void split_into(const float* dsrc, int rows, int K, bool kmajor, __bf16* out, const int* e2h = nullptr,
                bool frag = false) {
  long long ld, ps;
  plane_geom(rows, K, kmajor, ld, ps);
  SplitParams s{};
  s.x = dsrc;
  s.ldx = kmajor ? rows : K;
  s.rows = kmajor ? K : rows;
  s.cols = kmajor ? rows : K;
  s.out_rows = kmajor ? (int)up32(K) : rows;
  s.out = out;
  s.ldo = ld;
  s.po = ps;
  s.out_cols = (int)ld;
  s.e2h = e2h;
  s.frag = frag ? 1 : 0;
  split_planes(s, false, 1, nullptr);
}

__bf16* make_planes(DevBuf& db, const float* dsrc, int rows, int K, bool kmajor, long long& ld, long long& ps) {
  plane_geom(rows, K, kmajor, ld, ps);
  __bf16* out = db.get<__bf16>(3 * ps);
  if (out) split_into(dsrc, rows, K, kmajor, out);
  return out;
}

// Device buffers of the single-kernel DrQ entry points.  An output lies between two 256-byte bands
// of GUARD_BYTE and starts as all-ones words (NaN as float, -1 as int, 255 as byte), so a store
// outside it and an element the kernel left alone both show; the bands only detect.
constexpr size_t GUARD = 256;
constexpr int GUARD_BYTE = 0xA5;
struct Guarded {
  DevBuf mem;
  struct Out {
    unsigned char* raw;
    size_t bytes;
    const char* name;
  };
  std::vector<Out> outs;
  bool ok = true;
  template <typename T>
  T* in(const T* host, size_t n) {  // null host: no buffer
    if (!host) return nullptr;
    T* d = mem.get<T>(n);
    if (!d || hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  template <typename T>
  T* out(size_t n, const char* name) {
    const size_t bytes = n * sizeof(T);
    unsigned char* raw = mem.get<unsigned char>(bytes + 2 * GUARD);
    if (!raw || hipMemset(raw, GUARD_BYTE, bytes + 2 * GUARD) != hipSuccess ||
        hipMemset(raw + GUARD, 0xFF, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    outs.push_back({raw, bytes, name});
    return reinterpret_cast<T*>(raw + GUARD);
  }
  // 0, or -5 with the first written band named in mtsac_last_error
  int check() {
    unsigned char band[2 * GUARD];
    for (const Out& o : outs) {
      if (hipMemcpy(band, o.raw, GUARD, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(band + GUARD, o.raw + GUARD + o.bytes, GUARD, hipMemcpyDeviceToHost) != hipSuccess)
        return -5;
      for (size_t i = 0; i < 2 * GUARD; ++i)
        if (band[i] != GUARD_BYTE) {
          char msg[160];
          snprintf(msg, sizeof msg, "guard band written: buffer %s, %s band, byte %d", o.name,
                   i < GUARD ? "leading" : "trailing", (int)(i % GUARD));
          set_last_error(msg);
          return -5;
        }
    }
    return 0;
  }
  template <typename T>
  bool back(T* host, const T* dev, size_t n) {
    return hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
  }
};

// a guarded buffer that starts as the host's n values (in and out)
template <typename T>
T* guarded_inout(Guarded& g, const T* host, size_t n, const char* name) {
  T* d = g.out<T>(n, name);
  if (d && hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) g.ok = false;
  return d;
}

int sync_rc(const char* what) {
  const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
  if (e1 == hipSuccess && e2 == hipSuccess) return 0;
  set_last_error((std::string(what) + ": " + hipGetErrorString(e1 != hipSuccess ? e1 : e2)).c_str());
  return -5;
}

// ---- single SAC head kernels (heads.hip) ----
// counts / rows of task[B] from task_rows on the device (row stride B), both guarded outputs
struct TaskLists {
  int* d_task = nullptr;
  int* counts = nullptr;
  int* rows = nullptr;
  int max_count = 0;
};
bool tasks_ok(const int* task, int B, int T_l) {
  if (!task || B < 1 || T_l < 1 || T_l > 64) return false;
  for (int b = 0; b < B; ++b)
    if (task[b] < 0 || task[b] >= T_l) return false;
  return true;
}
// host output buffers of one call must not share a start address: each is copied back over whatever the
// one before it left there, so the caller would read one output under another's name (null entries skipped)
bool outputs_distinct(std::initializer_list<const void*> outs) {
  for (auto a = outs.begin(); a != outs.end(); ++a)
    for (auto b = a + 1; b != outs.end(); ++b)
      if (*a != nullptr && *a == *b) return false;
  return true;
}
TaskLists make_lists(Guarded& g, const int* task, int B, int T_l) {
  TaskLists l;
  std::vector<int> c(T_l, 0);
  for (int b = 0; b < B; ++b) l.max_count = std::max(l.max_count, ++c[task[b]]);
  l.d_task = g.in(task, (size_t)B);
  l.counts = g.out<int>((size_t)T_l, "counts");
  l.rows = g.out<int>((size_t)T_l * B, "rows");
  if (g.ok) task_rows(l.d_task, B, T_l, l.counts, l.rows, B, nullptr);
  return l;
}
// a guarded PlaneRec whose words start as all-ones (amax NaN); e set to `e`
PlaneRec* rec_out(Guarded& g, int e, const char* name) {
  PlaneRec* r = g.out<PlaneRec>(1, name);
  if (r && hipMemcpy(&r->e, &e, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) g.ok = false;
  return r;
}
// the unscaled sum of n elements' planes (16-bit words, plane stride ps): split3 h + m + l, split2h (h + l) 2^-e
bool planes_sum(const __bf16* dev, size_t n_words, size_t ps, size_t n, bool h2, int e, float* out) {
  std::vector<unsigned short> w(n_words);
  if (hipMemcpy(w.data(), dev, n_words * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
  for (size_t i = 0; i < n; ++i) {
    if (h2) {
      _Float16 a, b;
      std::memcpy(&a, &w[i], 2);
      std::memcpy(&b, &w[ps + i], 2);
      out[i] = std::ldexp((float)a + (float)b, -e);
    } else {
      __bf16 a, b, c;
      std::memcpy(&a, &w[i], 2);
      std::memcpy(&b, &w[ps + i], 2);
      std::memcpy(&c, &w[2 * ps + i], 2);
      out[i] = ((float)a + (float)b) + (float)c;
    }
  }
  return true;
}

// split2h test records: max |x| and the plane exponent of that bound, as plane_exp (gemm_common.h) gives it
float host_amax(const float* x, size_t n) {
  float m = 0.f;
  for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
  return m;
}
int host_plane_exp(float b) {
  b *= 1.00390625f;
  if (!(b > 0.f)) return 0;
  int ex;
  (void)std::frexp(b, &ex);
  return 15 - ex;
}

}  // namespace

extern "C" {

int mtsac_debug_gemm_x3p(int epi, int M, int N, int K, const float* A, int a_kmajor, const float* B, int b_kmajor,
                         float* C, const float* bias, const float* mask, float* Csum) {
  const int splits = (epi >> 8) & 255;
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || !A || !B || !C) return -22;
  DevBuf d;
  float* dA = d.get<float>((size_t)M * K);
  float* dB = d.get<float>((size_t)N * K);
  float* dC = d.get<float>((size_t)M * N);
  float* dbias = d.get<float>(N);
  float* dmask = d.get<float>((size_t)M * N);
  __bf16* dCp = d.get<__bf16>((size_t)3 * M * N);
  float* dws = d.get<float>(splits > 1 ? (size_t)gemm_ws_floats(M, N, 1, splits) : 1);
  if (!dA || !dB || !dC || !dbias || !dmask || !dCp || !dws) return -12;
  (void)hipMemcpy(dA, A, sizeof(float) * M * K, hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, B, sizeof(float) * N * K, hipMemcpyHostToDevice);
  if (bias) (void)hipMemcpy(dbias, bias, sizeof(float) * N, hipMemcpyHostToDevice);
  if (mask) (void)hipMemcpy(dmask, mask, sizeof(float) * M * N, hipMemcpyHostToDevice);
  long long lda, pa, ldb, pb;
  __bf16* Ap = make_planes(d, dA, M, K, a_kmajor != 0, lda, pa);
  __bf16* Bp = make_planes(d, dB, N, K, b_kmajor != 0, ldb, pb);
  if (!Ap || !Bp) return -12;
  SplitGemmParams g{};
  g.A = Ap; g.lda = lda; g.pA = pa; g.a_kmajor = a_kmajor != 0;
  g.B = Bp; g.ldb = ldb; g.pB = pb; g.b_kmajor = b_kmajor != 0;
  g.C = dC; g.ldc = N;
  g.bias = dbias;
  g.mask = dmask; g.ldm = N;
  if (Csum) {
    g.Cp = dCp; g.ldcp = N; g.pC = (long long)M * N;
  }
  g.M = M; g.N = N; g.K = (int)up32(K);
  g.splits = splits;
  g.ws = dws;
  gemm_x3p(g, epi, 1, nullptr);
  if (hipDeviceSynchronize() != hipSuccess) return -5;
  if (hipMemcpy(C, dC, sizeof(float) * M * N, hipMemcpyDeviceToHost) != hipSuccess) return -5;
  if (Csum) {
    std::vector<__bf16> h((size_t)3 * M * N);
    if (hipMemcpy(h.data(), dCp, sizeof(__bf16) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return -5;
    const size_t n = (size_t)M * N;
    for (size_t i = 0; i < n; ++i) Csum[i] = ((float)h[i] + (float)h[n + i]) + (float)h[2 * n + i];
  }
  return 0;
}

// the split2h k-major x k-major weight grad alone (mtsac_debug.h)
int mtsac_debug_gemm_x3p_kmajor(int E, int M, int N, int K, int slices, const float* A, const float* B, float* C) {
  if (E < 1 || E > 8 || M < 1 || N < 1 || K < 1 || slices < 1 || slices > 64 || slices > (int)(up32(K) / 32) || !A ||
      !B || !C || (long long)E * K * std::max(M, N) >= (1LL << 28))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const int Kp = (int)up32(K);
  long long lda, pa, ldb, pb;
  plane_geom(M, K, true, lda, pa);
  plane_geom(N, K, true, ldb, pb);
  // the operands' records as a producer leaves them: max |x| and the plane exponent of that bound
  PlaneRec hrec[2];
  std::memset(hrec, 0, sizeof hrec);
  const float ma = host_amax(A, (size_t)E * K * M), mb = host_amax(B, (size_t)E * K * N);
  hrec[0].e = host_plane_exp(ma); hrec[0].amax[0] = ma;
  hrec[1].e = host_plane_exp(mb); hrec[1].amax[0] = mb;
  Guarded gd;
  const PlaneRec* rec = gd.in(hrec, 2);
  const float *dA = gd.in(A, (size_t)E * K * M), *dB = gd.in(B, (size_t)E * K * N);
  __bf16* Ap = gd.mem.get<__bf16>((size_t)3 * pa * E);
  __bf16* Bp = gd.mem.get<__bf16>((size_t)3 * pb * E);
  float* dC = gd.out<float>((size_t)E * M * N, "C");  // starts as NaN between two guard bands
  float* ws = gd.mem.get<float>((size_t)std::max(gemm_ws_floats(M, N, E, std::max(slices, 2)), 1LL));
  if (!gd.ok || !Ap || !Bp || !ws) return -12;
  for (int z = 0; z < E; ++z) {
    split_into(dA + (size_t)z * K * M, M, K, true, Ap + 3 * pa * z, &rec[0].e);
    split_into(dB + (size_t)z * K * N, N, K, true, Bp + 3 * pb * z, &rec[1].e);
  }
  SplitGemmParams g{};
  g.np = 2;
  g.ra = rec; g.na = 1; g.rb = rec + 1; g.nb = 1;
  g.kmul = (float)K;
  g.A = Ap; g.lda = lda; g.pA = pa; g.sA = 3 * pa; g.a_kmajor = 1;
  g.B = Bp; g.ldb = ldb; g.pB = pb; g.sB = 3 * pb; g.b_kmajor = 1;
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.M = M; g.N = N; g.K = Kp;
  g.splits = slices;
  g.ws = ws;
  gemm_x3p(g, EPI_STORE, E, nullptr);
  int rc = 0;
  if ((rc = sync_rc("gemm_x3p k-major")) || (rc = gd.check())) return rc;
  return gd.back(C, dC, (size_t)E * M * N) ? 0 : -5;
}

int mtsac_debug_gemm_x3p_bench(int epi, int batch, int M, int N, int K, int iters, double* ms_per_launch) {
  const int layout = (epi >> 8) & 3;  // bit 0: A k-major, bit 1: B k-major
  const int splits = (epi >> 16) & 255;  // split-K slices (0/1: none; EPI_STORE: + splitk_reduce; 255: auto)
  const bool fin = (epi >> 12) & 1;      // arrival counters: the weight grads' in-launch reduce
  const bool h2 = (epi >> 13) & 1;       // precision split2h (zero exponents: operands in [-1, 1])
  const bool pout = (epi >> 14) & 1;     // output planes too (the forward's: bias+ReLU planes out)
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || iters < 1 || !ms_per_launch) return -22;
  DevBuf d;
  PlaneRec* rec = h2 ? d.get<PlaneRec>(3) : nullptr;
  float* fa = d.get<float>((size_t)M * K);
  float* fb = d.get<float>((size_t)N * K);
  float* C = d.get<float>((size_t)M * N * batch);
  float* bias = d.get<float>((size_t)N * batch);
  if (!fa || !fb || !C || !bias) return -12;
  hipLaunchKernelGGL(fill_rand_f32, dim3((unsigned)(((long long)M * K + 255) / 256)), dim3(256), 0, nullptr, fa,
                     (long long)M * K, 3u);
  hipLaunchKernelGGL(fill_rand_f32, dim3((unsigned)(((long long)N * K + 255) / 256)), dim3(256), 0, nullptr, fb,
                     (long long)N * K, 5u);
  // one plane set per batch entry (distinct memory, same values)
  long long lda, pa, ldb, pb;
  plane_geom(M, K, layout & 1, lda, pa);
  plane_geom(N, K, layout & 2, ldb, pb);
  __bf16* Ap = d.get<__bf16>((size_t)3 * pa * batch);
  __bf16* Bp = d.get<__bf16>((size_t)3 * pb * batch);
  if (!Ap || !Bp) return -12;
  for (int z = 0; z < batch; ++z) {
    split_into(fa, M, K, layout & 1, Ap + 3 * pa * z, h2 ? &rec[0].e : nullptr);
    split_into(fb, N, K, layout & 2, Bp + 3 * pb * z, h2 ? &rec[1].e : nullptr);
  }
  SplitGemmParams g{};
  if (h2) {
    g.np = 2;
    g.ra = rec; g.rb = rec + 1; g.rc = rec + 2;
    g.kmul = (float)K;
  }
  if (pout) {
    __bf16* Cp = d.get<__bf16>((size_t)3 * M * N * batch);
    if (!Cp) return -12;
    g.Cp = Cp; g.ldcp = N; g.pC = (long long)M * N; g.sCp = 3 * g.pC;
  }
  const bool planes_only = pout;
  g.A = Ap; g.lda = lda; g.pA = pa; g.sA = 3 * pa; g.a_kmajor = layout & 1;
  g.B = Bp; g.ldb = ldb; g.pB = pb; g.sB = 3 * pb; g.b_kmajor = (layout >> 1) & 1;
  g.C = planes_only ? nullptr : C; g.ldc = N; g.sC = (long long)M * N;
  g.bias = bias; g.sBias = N;
  g.mask = C; g.ldm = N; g.sMask = (long long)M * N;
  g.M = M; g.N = N; g.K = (int)up32(K);
  if (splits > 1) {
    g.splits = splits == 255 ? -1 : splits;
    const int sw = splits == 255 ? gemm_x3p_splits(M, N, g.K, batch, layout == 3) : splits;
    g.ws = d.get<float>((size_t)M * N * batch * std::max(sw, 1));
    if (!g.ws) return -12;
    if (fin) {
      g.cnt = d.get<int>((size_t)GEMM_X3F_CNT);
      if (!g.cnt) return -12;
    }
  }
  gemm_x3p(g, epi, batch, nullptr);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -5;
  (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters; ++i) gemm_x3p(g, epi, batch, nullptr);
  (void)hipEventRecord(e1, nullptr);
  if (hipEventSynchronize(e1) != hipSuccess) return -5;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return 0;
}

// gemm_x3f (row-major x row-major planes, K % 64 == 0): C[M][N] = A[M][K] . B[N][K]^T from host
// fp32 arrays, epi 1 bias+ReLU / 2 ReLU mask (fp32 mask, or with bit 8 of epi its bf16 high
// plane); Csum (nullable) receives the sum of the written planes.  -95 when gemm_x3f does not take
// the shape (too few tiles, layout).
int mtsac_debug_gemm_x3f(int epi, int batch, int M, int N, int K, const float* A, const float* B, float* C,
                         const float* bias, const float* mask, float* Csum) {
  const bool m16 = (epi >> 8) & 1;
  const bool small = (epi >> 9) & 1;  // gemm_x3s instead
  const int np = ((epi >> 10) & 1) ? 1 : 3;  // bf16: the high plane only
  const bool autosplit = (epi >> 11) & 1;     // split-K by the launcher's own choice (workspace given)
  const bool fin = (epi >> 12) & 1;           // ... with arrival counters: the in-launch finish
  const bool h2 = (epi >> 13) & 1;            // precision split2h: fp16 planes scaled per tensor
  const bool bfrag = (epi >> 14) & 1;         // B planes in the fragment layout (N % 16 == 0)
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || !A || !B || !C) return -22;
  if (bfrag && N % 16 != 0) return -22;
  DevBuf d;
  const size_t nA = (size_t)M * K * batch, nB = (size_t)N * K * batch, nC = (size_t)M * N * batch;
  // split2h: records of A, B (its max covering the bias, as a trunk record does), the mask and C
  PlaneRec* rec = d.get<PlaneRec>(4);
  if (!rec) return -12;
  if (h2) {
    auto amax = [](const float* x, size_t n) {
      float m = 0.f;
      for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
      return m;
    };
    auto pexp = [](float b) {
      b *= 1.00390625f;
      if (!(b > 0.f)) return 0;
      int ex;
      (void)std::frexp(b, &ex);
      return 15 - ex;
    };
    const float ma = amax(A, nA), mbias = (epi == 1 && bias) ? amax(bias, (size_t)N * batch) : 0.f;
    const float mb = std::max(amax(B, nB), mbias);
    const float mm = mask ? amax(mask, nC) : 1.f;
    std::vector<PlaneRec> h(4);
    std::memset(h.data(), 0, sizeof(PlaneRec) * 4);
    h[0].e = pexp(ma); h[0].amax[0] = ma;
    h[1].e = pexp(mb); h[1].amax[0] = mb;
    h[2].e = pexp(mm); h[2].amax[0] = mm;
    (void)hipMemcpy(rec, h.data(), sizeof(PlaneRec) * 4, hipMemcpyHostToDevice);
  }
  float* dA = d.get<float>(nA);
  float* dB = d.get<float>(nB);
  float* dC = d.get<float>(nC);
  float* dbias = d.get<float>((size_t)N * batch);
  float* dmask = d.get<float>(nC);
  __bf16* dCp = d.get<__bf16>(3 * nC);
  __bf16* dM16 = d.get<__bf16>(3 * nC);
  if (!dA || !dB || !dC || !dbias || !dmask || !dCp || !dM16) return -12;
  (void)hipMemcpy(dA, A, sizeof(float) * nA, hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, B, sizeof(float) * nB, hipMemcpyHostToDevice);
  if (bias) (void)hipMemcpy(dbias, bias, sizeof(float) * N * batch, hipMemcpyHostToDevice);
  if (mask) (void)hipMemcpy(dmask, mask, sizeof(float) * nC, hipMemcpyHostToDevice);
  const long long Kp = (K + 63) / 64 * 64;
  __bf16* Ap = d.get<__bf16>((size_t)3 * M * Kp * batch);
  __bf16* Bp = d.get<__bf16>((size_t)3 * N * Kp * batch);
  if (!Ap || !Bp) return -12;
  for (int z = 0; z < batch; ++z) {
    SplitParams s{};
    s.x = dA + (size_t)z * M * K; s.ldx = K; s.rows = M; s.cols = K;
    s.out = Ap + (size_t)z * 3 * M * Kp; s.ldo = Kp; s.po = (long long)M * Kp; s.out_rows = M; s.out_cols = (int)Kp;
    s.e2h = h2 ? &rec[0].e : nullptr;
    split_planes(s, false, 1, nullptr);
    s.x = dB + (size_t)z * N * K; s.rows = N;
    s.out = Bp + (size_t)z * 3 * N * Kp; s.po = (long long)N * Kp; s.out_rows = N;
    s.e2h = h2 ? &rec[1].e : nullptr;
    s.frag = bfrag ? 1 : 0;
    split_planes(s, false, 1, nullptr);
    s.frag = 0;
    if (m16) {  // planes of the mask, row stride N
      s.x = dmask + (size_t)z * M * N; s.ldx = N; s.rows = M; s.cols = N;
      s.out = dM16 + (size_t)z * 3 * M * N; s.ldo = N; s.po = (long long)M * N; s.out_rows = M; s.out_cols = N;
      s.e2h = h2 ? &rec[2].e : nullptr;
      split_planes(s, false, 1, nullptr);
    }
  }
  SplitGemmParams g{};
  g.A = Ap; g.lda = Kp; g.pA = (long long)M * Kp; g.sA = 3 * g.pA;
  g.B = Bp; g.ldb = Kp; g.pB = (long long)N * Kp; g.sB = 3 * g.pB;
  g.b_frag = bfrag ? 1 : 0;
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.bias = dbias; g.sBias = N;
  g.mask = dmask; g.ldm = N; g.sMask = (long long)M * N;
  if (m16) {
    g.mask16 = dM16;
    g.sMask = 3ll * M * N;
  }
  if (Csum) {
    g.Cp = dCp; g.ldcp = N; g.pC = (long long)M * N; g.sCp = 3 * g.pC;
  }
  g.M = M; g.N = N; g.K = (int)Kp;
  g.np = h2 ? 2 : np;
  if (h2) {
    g.ra = rec + 0; g.na = 1;
    g.rb = rec + 1; g.nb = 1;
    g.rc = rec + 3;
    g.bias_in_b = epi == 1 && bias ? 1 : 0;
    g.pMask = (long long)M * N;
    g.kmul = (float)K;
  }
  if (autosplit) {
    g.ws = d.get<float>((size_t)std::max(gemm_x3f_ws_floats(M, N, (int)Kp, batch), 1LL));
    if (!g.ws) return -12;
    g.splits = -1;
    if (fin) {
      g.cnt = d.get<int>((size_t)GEMM_X3F_CNT);
      if (!g.cnt || hipMemset(g.cnt, 0, sizeof(int) * GEMM_X3F_CNT) != hipSuccess) return -12;
    }
  }
  if (small) {
    if (!gemm_x3s_ok(g, epi, batch)) return -95;
    gemm_x3s(g, epi, batch, nullptr);
  } else {
    if (!gemm_x3f_ok(g, epi, batch)) return -95;
    gemm_x3f(g, epi, batch, nullptr);
  }
  {
    const hipError_t le = hipGetLastError();  // a launch the runtime refused leaves C as it was
    if (le != hipSuccess) {
      fprintf(stderr, "[mtsac_debug_gemm_x3f] launch refused: %s\n", hipGetErrorString(le));
      return -6;
    }
  }
  if (hipDeviceSynchronize() != hipSuccess) return -5;
  if (hipMemcpy(C, dC, sizeof(float) * nC, hipMemcpyDeviceToHost) != hipSuccess) return -5;
  if (Csum && h2) {  // (h + l) 2^-ec
    std::vector<_Float16> h(3 * nC);
    int ec = 0;
    if (hipMemcpy(h.data(), dCp, sizeof(_Float16) * h.size(), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&ec, &rec[3].e, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return -5;
    const size_t n = (size_t)M * N;
    for (int z = 0; z < batch; ++z)
      for (size_t i = 0; i < n; ++i) {
        const _Float16* q = &h[(size_t)z * 3 * n];
        Csum[(size_t)z * n + i] = std::ldexp((float)q[i] + (float)q[n + i], -ec);
      }
  } else if (Csum) {
    std::vector<__bf16> h(3 * nC);
    if (hipMemcpy(h.data(), dCp, sizeof(__bf16) * h.size(), hipMemcpyDeviceToHost) != hipSuccess) return -5;
    const size_t n = (size_t)M * N;
    for (int z = 0; z < batch; ++z)
      for (size_t i = 0; i < n; ++i) {
        const __bf16* q = &h[(size_t)z * 3 * n];
        Csum[(size_t)z * n + i] = ((float)q[i] + (float)q[n + i]) + (float)q[2 * n + i];
      }
  }
  return 0;
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
  // records: A, W, mask, dense out, ragged out
  auto amax = [](const float* x, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
    return m;
  };
  auto pexp = [](float b) {
    b *= 1.00390625f;
    if (!(b > 0.f)) return 0;
    int ex;
    (void)std::frexp(b, &ex);
    return 15 - ex;
  };
  std::vector<PlaneRec> hrec(5);
  std::memset(hrec.data(), 0, sizeof(PlaneRec) * hrec.size());
  const float ma = amax(Az.data(), nA), mw = amax(W, nW), mm = amax(mask, nC);
  hrec[0].e = pexp(ma); hrec[0].amax[0] = ma;
  hrec[1].e = pexp(mw); hrec[1].amax[0] = mw;
  hrec[2].e = pexp(mm); hrec[2].amax[0] = mm;
  hrec[3].e = hrec[4].e = 0x7fffffff;
  for (int i = 0; i < PLANE_REC_PARTS; ++i) hrec[3].amax[i] = hrec[4].amax[i] = 1e30f;  // poison: a stale slot shows
  PlaneRec* rec = gd.in(hrec.data(), hrec.size());
  const long long Kp = (K + 63) / 64 * 64;
  __bf16* Azp = gd.mem.get<__bf16>((size_t)3 * B * Kp * E);
  __bf16* Acp = gd.mem.get<__bf16>((size_t)3 * B * Kp * E);
  __bf16* Wp = gd.mem.get<__bf16>((size_t)3 * N * Kp * E);
  __bf16* Mp = gd.mem.get<__bf16>(3 * nC);
  const size_t out_bytes = pout ? nC * 2 * sizeof(__bf16) : nC * sizeof(float);
  unsigned char* dden = gd.out<unsigned char>(out_bytes, "dense out");
  unsigned char* drag = gd.out<unsigned char>(out_bytes, "ragged out");
  if (!gd.ok || !dAc || !rec || !Azp || !Acp || !Wp || !Mp) return -12;
  for (int z = 0; z < E; ++z) {
    SplitParams sp{};
    sp.ldx = K; sp.rows = B; sp.cols = K; sp.ldo = Kp; sp.po = (long long)B * Kp; sp.out_rows = B; sp.out_cols = (int)Kp;
    sp.e2h = &rec[0].e;
    sp.x = dAz + (size_t)z * B * K; sp.out = Azp + (size_t)z * 3 * B * Kp;
    split_planes(sp, false, 1, nullptr);
    sp.x = dAc + (size_t)z * B * K; sp.out = Acp + (size_t)z * 3 * B * Kp;
    split_planes(sp, false, 1, nullptr);
    sp.x = dW + (size_t)z * N * K; sp.rows = N; sp.out = Wp + (size_t)z * 3 * N * Kp; sp.po = (long long)N * Kp;
    sp.out_rows = N; sp.e2h = &rec[1].e; sp.frag = bfrag ? 1 : 0;
    split_planes(sp, false, 1, nullptr);
    sp.frag = 0;
    sp.x = dmask + (size_t)z * B * N; sp.ldx = N; sp.rows = B; sp.cols = N;
    sp.out = Mp + (size_t)z * 3 * B * N; sp.ldo = N; sp.po = (long long)B * N; sp.out_rows = B; sp.out_cols = N;
    sp.e2h = &rec[2].e;
    split_planes(sp, false, 1, nullptr);
  }
  SplitGemmParams g{};
  g.np = 2;
  g.lda = Kp; g.pA = (long long)B * Kp; g.sA = 3 * g.pA;
  g.B = Wp; g.ldb = Kp; g.pB = (long long)N * Kp; g.sB = 3 * g.pB;
  g.b_frag = bfrag ? 1 : 0;
  g.mask16 = Mp; g.ldm = N; g.sMask = 3ll * B * N; g.pMask = (long long)B * N;
  g.M = B; g.N = N; g.K = (int)Kp;
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
  g.A = Azp;
  outs(dden, rec + 3, &nparts[0]);
  gemm_x3f(g, EPI_RELU_MASK, E, nullptr);  // no workspace: the plain unsplit launch
  if (int rc = sync_rc("dense gemm_x3f")) return rc;
  g.A = Acp;
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
  const int outs = (epi >> 8) & 3;  // 0: fp32 + planes, 1: planes only, 2: fp32 only
  const int np = ((epi >> 10) & 1) ? 1 : 3;  // bf16: the high plane only
  const bool autosplit = (epi >> 11) & 1;     // split-K by the launcher's own choice (workspace given)
  const bool fin = (epi >> 12) & 1;           // ... with arrival counters: the in-launch finish
  const bool h2 = (epi >> 13) & 1;            // precision split2h (exponents 0: operands in [-1, 1])
  const bool bfrag = (epi >> 14) & 1;         // gemm_x3f: B planes in the fragment layout
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || iters < 1 || !ms_per_launch) return -22;
  DevBuf d;
  const long long Kp = (K + 63) / 64 * 64;
  PlaneRec* rec = d.get<PlaneRec>(3);  // zero exponents: the random operands lie in [-1, 1]
  if (!rec) return -12;
  float* fa = d.get<float>((size_t)M * Kp);
  float* fb = d.get<float>((size_t)N * Kp);
  float* C = d.get<float>((size_t)M * N * batch);
  float* bias = d.get<float>((size_t)N * batch);
  __bf16* Cp = d.get<__bf16>((size_t)3 * M * N * batch);
  if (!fa || !fb || !C || !bias || !Cp) return -12;
  hipLaunchKernelGGL(fill_rand_f32, dim3((unsigned)(((long long)M * Kp + 255) / 256)), dim3(256), 0, nullptr, fa,
                     (long long)M * Kp, 3u);
  hipLaunchKernelGGL(fill_rand_f32, dim3((unsigned)(((long long)N * Kp + 255) / 256)), dim3(256), 0, nullptr, fb,
                     (long long)N * Kp, 5u);
  const bool bk = which == 0;  // gemm_x3p forward: B k-major [K][N]
  long long lda, pa, ldb, pb;
  plane_geom(M, (int)Kp, false, lda, pa);
  plane_geom(N, (int)Kp, bk, ldb, pb);
  __bf16* Ap = d.get<__bf16>((size_t)3 * pa * batch);
  __bf16* Bp = d.get<__bf16>((size_t)3 * pb * batch);
  if (!Ap || !Bp) return -12;
  for (int z = 0; z < batch; ++z) {
    split_into(fa, M, (int)Kp, false, Ap + 3 * pa * z, h2 ? &rec[0].e : nullptr);
    split_into(fb, N, (int)Kp, bk, Bp + 3 * pb * z, h2 ? &rec[1].e : nullptr, bfrag && !bk);
  }
  SplitGemmParams g{};
  if (h2) {
    g.ra = rec; g.rb = rec + 1; g.rc = rec + 2;
    g.kmul = (float)K;
    g.pMask = (long long)M * N;
  }
  g.A = Ap; g.lda = lda; g.pA = pa; g.sA = 3 * pa;
  g.B = Bp; g.ldb = ldb; g.pB = pb; g.sB = 3 * pb; g.b_kmajor = bk;
  g.b_frag = bfrag && !bk ? 1 : 0;
  g.C = C; g.ldc = N; g.sC = (long long)M * N;
  g.bias = bias; g.sBias = N;
  g.mask = C; g.ldm = N; g.sMask = (long long)M * N;
  g.Cp = Cp; g.ldcp = N; g.pC = (long long)M * N; g.sCp = 3 * g.pC;
  if (outs == 1) g.C = nullptr;
  if (outs == 2) g.Cp = nullptr;
  g.M = M; g.N = N; g.K = (int)Kp;
  g.splits = 1;
  g.np = h2 ? 2 : np;
  if (autosplit) {
    const long long wsf = std::max(gemm_x3f_ws_floats(M, N, (int)Kp, batch), gemm_x3p_ws_floats(M, N, (int)Kp, batch, false));
    g.ws = d.get<float>((size_t)std::max(wsf, 1LL));
    if (!g.ws) return -12;
    g.splits = -1;
    if (fin) {
      g.cnt = d.get<int>((size_t)GEMM_X3F_CNT);
      if (!g.cnt) return -12;
    }
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
  run();
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -5;
  (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters; ++i) run();
  (void)hipEventRecord(e1, nullptr);
  if (hipEventSynchronize(e1) != hipSuccess) return -5;
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return 0;
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

// DrQ conv channel groups per lane (0 = the engine's choice); returns the previous fwd | bwd << 8
int mtsac_debug_drq_groups(int fwd, int bwd) {
  const int old = drq::g_drq_fwd_g | (drq::g_drq_bwd_g << 8);
  drq::g_drq_fwd_g = fwd;
  drq::g_drq_bwd_g = bwd;
  return old;
}

// DrQ convs on f32 MFMA (bit 1 forward, 2 data grad, 4 weight grad) or the VALU kernels; returns the
// previous mask (< 0: query only)
int mtsac_debug_drq_mfma(int mask) {
  const int old = drq::g_drq_mfma;
  if (mask >= 0) drq::g_drq_mfma = mask & 7;
  return old;
}

// the pre-round-6 DrQ conv kernels (bit 1 forward, 2 data grad, 4 weight grad) or the row-tile ones;
// returns the previous mask (< 0: query only)
int mtsac_debug_drq_legacy(int mask) {
  const int old = drq::g_drq_legacy;
  if (mask >= 0) drq::g_drq_legacy = mask & 63;
  return old;
}

// the row-tile conv weight grad's grid cap (> 0 sets, 0 restores the per-shape default; < 0 queries;
// returns the previous); engines created before a change keep partial buffers sized for the old cap,
// so set it before creating one (experiments)
int mtsac_debug_drq_wgrad_blocks(int cap) {
  const int old = drq::g_drq_wg_blocks;
  if (cap >= 0) drq::g_drq_wg_blocks = cap;
  return old;
}

// mean microseconds per launch of one DrQ conv pass on random operands (drq::conv_bench)
int mtsac_debug_drq_conv_bench(int kind, int B, int H, int W, int ci, int co, int iters, double* us_per_launch) {
  if (kind < 0 || kind > 2 || B < 1 || H < 1 || W < 1 || iters < 1 || !us_per_launch || !drq::conv_supported(ci, co))
    return -22;
  const double us = drq::conv_bench(kind, B, H, W, ci, co, iters);
  if (us < 0) return -12;
  *us_per_launch = us;
  return hipDeviceSynchronize() == hipSuccess ? 0 : -5;
}

// what the conv launcher of `kind` runs at this shape under the current masks (drq::conv_path)
int mtsac_debug_drq_conv_path(int kind, int B, int H, int W, int ci, int co, int* out) {
  if (kind < 0 || kind > 2 || B < 1 || H < 1 || W < 1 || !out || !drq::conv_supported(ci, co) ||
      (long long)B * H * W * 16 >= (1LL << 31))
    return -22;
  const drq::ConvPath p = drq::conv_path(kind, B, H, W, ci, co);
  out[0] = p.family;
  out[1] = p.R;
  out[2] = p.n;
  out[3] = p.blocks;
  return 0;
}

// one conv pass as the engine launches it, host pointers in and out (mtsac_debug.h)
int mtsac_debug_drq_conv(int kind, int flags, int B, int B1, int H, int W, int ci, int co, const float* x,
                         const float* w, const float* bias, const float* w2, const float* bias2, const float* aux,
                         const float* aux2, float* out, float* out2) {
  if (kind < 0 || kind > 2 || (flags & ~3) || B < 1 || H < 1 || W < 1 || !x || (kind != 2 && !w) || !out ||
      !drq::conv_supported(ci, co) || (long long)B * H * W * 16 >= (1LL << 31))
    return -22;
  if (kind == 0 && (!bias || (w2 != nullptr) != (bias2 != nullptr) || (w2 && (B1 < 0 || B1 > B)) || (flags & 2)))
    return -22;
  if (kind == 1 && flags) return -22;
  if (kind == 2 && (!aux || !out2)) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t np = (size_t)B * H * W, nw = (size_t)9 * ci * co;
  Guarded g;
  int rc = 0;
  if (kind == 0) {
    const float* dx = g.in(x, np * ci);
    const float *dw = g.in(w, nw), *dbi = g.in(bias, (size_t)co), *dw2 = g.in(w2, nw), *db2 = g.in(bias2, (size_t)co);
    const float* dres = g.in(aux, np * co);
    float* dout = g.out<float>(np * co, "out");
    if (!g.ok) return -12;
    drq::conv_fwd(dx, dw, dbi, dres, dout, B, H, W, ci, co, (flags & 1) != 0, nullptr, dw2, db2, w2 ? B1 : -1);
    if ((rc = sync_rc("conv_fwd")) || (rc = g.check())) return rc;
    if (!g.back(out, dout, np * co)) return -5;
  } else if (kind == 1) {
    const float *ddout = g.in(x, np * co), *dw = g.in(w, nw), *dmask = g.in(aux, np * ci), *ddres = g.in(aux2, np * ci);
    float* ddin = g.out<float>(np * ci, "din");
    if (!g.ok) return -12;
    drq::conv_bwd_data(ddout, dw, dmask, ddres, ddin, B, H, W, ci, co, nullptr);
    if ((rc = sync_rc("conv_bwd_data")) || (rc = g.check())) return rc;
    if (!g.back(out, ddin, np * ci)) return -5;
  } else {
    const int G = drq::conv_wgrad_blocks(B, H, W, ci, co), n = (int)nw + co;
    const bool defer = (flags & 2) != 0;
    const float *dx = g.in(x, np * ci), *ddout = g.in(aux, np * co);
    float* part = g.out<float>((size_t)G * n, "part");
    float* ddw = g.out<float>(nw, "dw");
    float* ddb = g.out<float>((size_t)co, "db");
    if (!g.ok) return -12;
    const drq::SumSeg seg{part, ddw, ddb, G, n, (int)nw, 0};
    const drq::SumSeg* dseg = g.in(&seg, 1);
    if (!g.ok) return -12;
    drq::conv_wgrad(dx, ddout, part, ddw, ddb, B, H, W, ci, co, (flags & 1) != 0, nullptr, defer);
    if (defer) drq::sum_parts_multi(dseg, 1, drq::sum_parts_blocks(ci, co), nullptr);
    if ((rc = sync_rc("conv_wgrad")) || (rc = g.check())) return rc;
    if (!g.back(out, ddw, nw) || !g.back(out2, ddb, (size_t)co)) return -5;
  }
  return 0;
}

// maxpool_fwd then maxpool_bwd (3 x 3 / stride 2 / SAME, NHWC): out, arg [B][Ho][Wo][C], din [B][H][W][C]
int mtsac_debug_drq_maxpool(int B, int H, int W, int C, const float* in, float* out, unsigned char* arg,
                            const float* dout, float* din) {
  if (B < 1 || H < 1 || W < 1 || C < 4 || C % 4 || !in || !out || !arg || !dout || !din ||
      (long long)B * H * W * C >= (1LL << 31))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t ni = (size_t)B * H * W * C, no = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * C;
  Guarded g;
  const float *d_in = g.in(in, ni), *d_dout = g.in(dout, no);
  float* d_out = g.out<float>(no, "out");
  unsigned char* d_arg = g.out<unsigned char>(no, "arg");
  float* d_din = g.out<float>(ni, "din");
  if (!g.ok) return -12;
  drq::maxpool_fwd(d_in, d_out, d_arg, B, H, W, C, nullptr);
  drq::maxpool_bwd(d_dout, d_arg, d_din, B, H, W, C, nullptr);
  int rc = 0;
  if ((rc = sync_rc("maxpool")) || (rc = g.check())) return rc;
  return g.back(out, d_out, no) && g.back(arg, d_arg, no) && g.back(din, d_din, ni) ? 0 : -5;
}

// c51_target(hc_n, hc_t) -> m, a_next; q_values(hc_n) -> q; c51_loss(hc_s, m) -> dh, loss_b, logit_b
int mtsac_debug_drq_c51(int B, int A, int Z, int ldh, const float* hc_s, const float* hc_n, const float* hc_t,
                        const float* hb_on, const float* hb_tg, const float* rew, const float* done, const int* act,
                        float gamma_n, float vmin, float vmax, float* m, int* a_next, float* q, float* dh,
                        float* loss_b, float* logit_b) {
  if (B < 1 || A < 1 || Z < 2 || Z > 64 || ldh < (A + 1) * Z || !(vmax > vmin) || !hc_s || !hc_n || !hc_t || !hb_on ||
      !hb_tg || !rew || !done || !act || !m || !a_next || !q || !dh || !loss_b || !logit_b ||
      (long long)B * ldh >= (1LL << 31))
    return -22;
  for (int b = 0; b < B; ++b)
    if (act[b] < 0 || act[b] >= A) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t nh = (size_t)B * ldh, nb = (size_t)(A + 1) * Z;
  Guarded g;
  const float *d_s = g.in(hc_s, nh), *d_n = g.in(hc_n, nh), *d_t = g.in(hc_t, nh);
  const float *d_bon = g.in(hb_on, nb), *d_btg = g.in(hb_tg, nb), *d_rew = g.in(rew, (size_t)B), *d_done = g.in(done, (size_t)B);
  const int* d_act = g.in(act, (size_t)B);
  float* d_m = g.out<float>((size_t)B * Z, "m");
  int* d_an = g.out<int>((size_t)B, "a_next");
  float* d_q = g.out<float>((size_t)B * A, "q");
  float* d_dh = g.out<float>(nh, "dh");
  float* d_lb = g.out<float>((size_t)B, "loss_b");
  float* d_gb = g.out<float>((size_t)B, "logit_b");
  if (!g.ok) return -12;
  drq::c51_target(d_n, d_t, ldh, d_bon, d_btg, A, Z, d_rew, d_done, gamma_n, vmin, vmax, d_m, d_an, B, nullptr);
  drq::q_values(d_n, ldh, d_bon, A, Z, vmin, vmax, d_q, B, nullptr);
  drq::c51_loss(d_s, ldh, d_bon, A, Z, d_act, d_m, d_dh, d_lb, d_gb, B, nullptr);
  int rc = 0;
  if ((rc = sync_rc("c51")) || (rc = g.check())) return rc;
  return g.back(m, d_m, (size_t)B * Z) && g.back(a_next, d_an, (size_t)B) && g.back(q, d_q, (size_t)B * A) &&
                 g.back(dh, d_dh, nh) && g.back(loss_b, d_lb, (size_t)B) && g.back(logit_b, d_gb, (size_t)B)
             ? 0
             : -5;
}

int mtsac_debug_head_rw(int rw) {
  const int old = g_head_rw;
  g_head_rw = rw == 1 || rw == 2 || rw == 4 ? rw : -1;
  return old;
}

int mtsac_debug_head_bwd_split(int mode) {
  const int old = g_head_bwd_split;
  g_head_bwd_split = mode == 0 || mode == 1 ? mode : -1;
  return old;
}

// eps given: injected noise; eps null: the device stream (seed, stream_id + s for row set s, counter, noise_div)
static int head_policy_run(int form, int flags, int B, int T_l, int W, int A, int ld_a, const int* task, const float* h,
                           const float* Wh, const float* bh, const float* eps, unsigned long long seed,
                           unsigned int stream_id, unsigned long long counter, int noise_div, float ls_min,
                           float ls_max, float* a_out, float* a_out2, float* logpi, float* cache, float* planes,
                           int* counts, int* rows) {
  const bool whT = flags & 1, p3 = flags & 2, p2h = flags & 4;
  if (form < 0 || form > 2 || (flags & ~7) || (p3 && p2h) || W < 1 || A < 1 || A > 64 || !head_kernels_cover(2 * A, W) || ld_a < A || !h || !Wh || !bh ||
      noise_div < 0 || !a_out || !a_out2 || !logpi || !cache || !counts || !rows || ((p3 || p2h) && !planes) ||
      !tasks_ok(task, B, T_l) || (long long)B * W >= (1LL << 28) ||
      !outputs_distinct({a_out, a_out2, logpi, cache, planes, counts, rows}))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const int hd = 2 * A, ns = form == 2 ? 2 : 1, H2E = 14;  // |a| <= 1 at 2^14 fits fp16
  const size_t nw = (size_t)T_l * W * hd, npl = (p2h ? 2 : 3) * (size_t)B * ld_a;
  Guarded g;
  TaskLists tl = make_lists(g, task, B, T_l);
  const float *d_h = g.in(h, (size_t)ns * B * W), *d_Wh = g.in(Wh, nw), *d_bh = g.in(bh, (size_t)T_l * hd);
  const float* d_eps = g.in(eps, (size_t)ns * B * A);
  const unsigned long long* d_counter = g.in(&counter, 1);
  float* d_WhT = whT ? g.out<float>(nw, "WhT") : nullptr;
  PlaneRec* rec = p2h ? rec_out(g, H2E, "ap_rec") : nullptr;
  float *d_a[2], *d_a2[2], *d_lp[2], *d_c[2];
  __bf16* d_pl[2] = {nullptr, nullptr};
  for (int s = 0; s < ns; ++s) {
    d_a[s] = g.out<float>((size_t)B * ld_a, "a_out");
    d_a2[s] = g.out<float>((size_t)B * ld_a, "a_out2");
    d_lp[s] = g.out<float>((size_t)B, "logpi");
    d_c[s] = g.out<float>((size_t)B * 5 * A, "cache");
    if (p3 || p2h) d_pl[s] = g.out<__bf16>(npl, "a_planes");
  }
  if (!g.ok) return -12;
  if (whT) head_transpose(d_Wh, T_l, W, hd, d_WhT, nullptr);
  PolicyParams pp[2];
  for (int s = 0; s < ns; ++s) {
    PolicyParams p{};
    p.head.h = d_h + (size_t)s * B * W; p.head.Wh = d_Wh; p.head.WhT = d_WhT; p.head.bh = d_bh; p.head.task = tl.d_task;
    p.head.B = B; p.head.W = W; p.head.hd = hd; p.head.E = 1;
    p.eps = d_eps ? d_eps + (size_t)s * B * A : nullptr;
    p.seed = seed; p.counter = d_counter; p.stream_id = stream_id + (unsigned)s; p.noise_div = noise_div;
    p.A = A; p.ls_min = ls_min; p.ls_max = ls_max;
    p.a_out = d_a[s]; p.ld_a_out = ld_a; p.a_out2 = d_a2[s]; p.ld_a_out2 = ld_a;
    p.a_planes = d_pl[s]; p.ap_ps = (long long)B * ld_a; p.ap_ld = ld_a; p.ap_rec = rec;
    p.logpi = d_lp[s]; p.cache = d_c[s];
    if (form != 0) {
      p.counts = tl.counts; p.rows = tl.rows; p.max_rows = B; p.T_l = T_l; p.max_count = tl.max_count;
    }
    pp[s] = p;
  }
  if (!(form == 2 ? policy_head_pair(pp[0], pp[1], nullptr) : policy_head(pp[0], nullptr))) return -22;
  int rc = 0;
  if ((rc = sync_rc("policy_head")) || (rc = g.check())) return rc;
  for (int s = 0; s < ns; ++s) {
    if (!g.back(a_out + (size_t)s * B * ld_a, d_a[s], (size_t)B * ld_a) ||
        !g.back(a_out2 + (size_t)s * B * ld_a, d_a2[s], (size_t)B * ld_a) || !g.back(logpi + (size_t)s * B, d_lp[s], (size_t)B) ||
        !g.back(cache + (size_t)s * B * 5 * A, d_c[s], (size_t)B * 5 * A))
      return -5;
    if (d_pl[s] && !planes_sum(d_pl[s], npl, (size_t)B * ld_a, (size_t)B * ld_a, p2h, H2E, planes + (size_t)s * B * ld_a))
      return -5;
  }
  return g.back(counts, tl.counts, (size_t)T_l) && g.back(rows, tl.rows, (size_t)T_l * B) ? 0 : -5;
}

int mtsac_debug_head_policy(int form, int flags, int B, int T_l, int W, int A, int ld_a, const int* task, const float* h,
                            const float* Wh, const float* bh, const float* eps, float ls_min, float ls_max,
                            float* a_out, float* a_out2, float* logpi, float* cache, float* planes, int* counts,
                            int* rows) {
  if (!eps) return -22;
  return head_policy_run(form, flags, B, T_l, W, A, ld_a, task, h, Wh, bh, eps, 0ull, 0u, 0ull, 0, ls_min, ls_max, a_out,
                         a_out2, logpi, cache, planes, counts, rows);
}

int mtsac_debug_head_policy_noise(int form, int flags, int B, int T_l, int W, int A, int ld_a, const int* task,
                                  const float* h, const float* Wh, const float* bh, uint64_t seed, uint32_t stream_id,
                                  uint64_t counter, int noise_div, float ls_min, float ls_max, float* a_out,
                                  float* a_out2, float* logpi, float* cache, float* planes, int* counts, int* rows) {
  return head_policy_run(form, flags, B, T_l, W, A, ld_a, task, h, Wh, bh, nullptr, seed, stream_id, counter, noise_div,
                         ls_min, ls_max, a_out, a_out2, logpi, cache, planes, counts, rows);
}

int mtsac_debug_head_critic(int mode, int flags, int B, int T_l, int E, int W, int T_glob, int task_begin,
                            const int* task, const float* h, const float* Wh, const float* bh, const float* th,
                            const float* tWh, const float* tbh, const float* rew, const float* done,
                            const float* logpi, const float* log_alpha, const float* y, const float* tw, float gamma,
                            float inv_norm, float* y_out, float* dq, float* row_a, float* row_b, float* alpha_w,
                            float* dq_amax, int* dq_parts) {
  const bool fused = flags & 1, clip = flags & 2;
  if (mode < 0 || mode > 2 || (flags & ~3) || E < 1 || E > 4 || W < 1 || task_begin < 0 || T_glob < task_begin + T_l ||
      !h || !Wh || !bh || !rew || !done || !logpi || !log_alpha || !y_out || !dq || !row_a || !row_b || !alpha_w ||
      !dq_amax || !dq_parts || (fused && (mode != CH_CRITIC || !th || !tWh || !tbh)) ||
      (mode == CH_CRITIC && !fused && !y) || !tasks_ok(task, B, T_l) || (long long)E * B * W >= (1LL << 28))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t nh = (size_t)E * B * W, nw = (size_t)E * T_l * W, nb = (size_t)E * T_l;
  Guarded g;
  const int* d_task = g.in(task, (size_t)B);
  CriticHeadParams p{};
  auto head = [&](const float* hh, const float* ww, const float* bb) {
    HeadParams q{};
    q.h = g.in(hh, nh); q.Wh = g.in(ww, nw); q.bh = g.in(bb, nb); q.task = d_task;
    q.B = B; q.W = W; q.hd = 1; q.E = E;
    q.sWh = (long long)T_l * W; q.sbh = T_l; q.sh = (long long)B * W;
    return q;
  };
  p.head = head(h, Wh, bh);
  if (fused) p.thead = head(th, tWh, tbh);
  p.mode = mode; p.fused_target = fused; p.clip = clip;
  p.rew = g.in(rew, (size_t)B); p.done = g.in(done, (size_t)B); p.logpi = g.in(logpi, (size_t)B);
  p.log_alpha = g.in(log_alpha, (size_t)T_glob); p.task = d_task; p.task_begin = task_begin;
  p.y = g.in(y, (size_t)B); p.tw = g.in(tw, (size_t)B);
  p.y_out = g.out<float>((size_t)B, "y_out");
  p.dq = g.out<float>((size_t)E * B, "dq");
  p.row_a = g.out<float>((size_t)B, "row_a");
  p.row_b = g.out<float>((size_t)B, "row_b");
  p.alpha_w = g.out<float>((size_t)B, "alpha_w");
  p.dq_rec = rec_out(g, 0, "dq_rec");
  p.gamma = gamma; p.use_task_weights = tw != nullptr; p.T_glob = T_glob; p.inv_norm = inv_norm;
  int parts = -1;
  p.dq_parts = &parts;
  if (!g.ok) return -12;
  critic_head(p, nullptr);
  int rc = 0;
  if ((rc = sync_rc("critic_head")) || (rc = g.check())) return rc;
  *dq_parts = parts;
  return g.back(y_out, p.y_out, (size_t)B) && g.back(dq, p.dq, (size_t)E * B) && g.back(row_a, p.row_a, (size_t)B) &&
                 g.back(row_b, p.row_b, (size_t)B) && g.back(alpha_w, p.alpha_w, (size_t)B) &&
                 g.back(dq_amax, p.dq_rec->amax, (size_t)PLANE_REC_PARTS)
             ? 0
             : -5;
}

int mtsac_debug_head_active_rows(int E, int B, const float* dq, int* n, int* rows, int* slot) {
  if (E < 1 || E > 4 || B < 1 || !dq || !n || !rows || !slot) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const float* d_dq = g.in(dq, (size_t)E * B);
  int* d_n = g.out<int>((size_t)E, "n");
  int* d_rows = g.out<int>((size_t)E * B, "rows");
  int* d_slot = g.out<int>((size_t)E * B, "slot");
  if (!g.ok) return -12;
  active_rows(d_dq, E, B, d_n, d_rows, d_slot, nullptr);
  int rc = 0;
  if ((rc = sync_rc("active_rows")) || (rc = g.check())) return rc;
  return g.back(n, d_n, (size_t)E) && g.back(rows, d_rows, (size_t)E * B) && g.back(slot, d_slot, (size_t)E * B) ? 0 : -5;
}

// ---- the network-metrics kernels (netmetrics.hip) ----
// H [Z][M][ld] on the device, followed by M rows of NaN (a read past the last matrix shows in the results)
static float* metrics_input(Guarded& g, const float* H, int Z, int M, int ld) {
  const size_t n = (size_t)Z * M * ld, tail = (size_t)M * ld;
  float* d = g.mem.get<float>(n + tail);
  if (!d || hipMemcpy(d, H, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d + n, 0xFF, tail * sizeof(float)) != hipSuccess)
    g.ok = false;
  return d;
}

int mtsac_debug_act_stats(int Z, int M, int W, int ld, const float* H, float threshold, float* score, float* norm,
                          int32_t* count) {
  if (Z < 1 || Z > 64 || M < 1 || W < 1 || ld < W || !H || !score || !norm || !count || !std::isfinite(threshold))
    return -22;
  if (!outputs_distinct({score, norm, count})) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  ActStats s{};
  s.H = metrics_input(g, H, Z, M, ld);
  s.Z = Z;
  s.M = M;
  s.W = W;
  s.ld = ld;
  s.sH = (long long)M * ld;
  s.threshold = threshold;
  s.part = g.out<double>((size_t)Z * act_stats_chunks(M) * W, "part");
  s.score = g.out<float>((size_t)Z * W, "score");
  s.s_score = W;
  s.norm = g.out<float>((size_t)Z * W, "norm");
  s.s_norm = W;
  s.count = g.out<int>((size_t)Z, "count");
  s.s_count = 1;
  if (!g.ok) return -12;
  act_stats(s, nullptr);
  int rc = 0;
  if ((rc = sync_rc("act_stats")) || (rc = g.check())) return rc;
  return g.back(score, s.score, (size_t)Z * W) && g.back(norm, s.norm, (size_t)Z * W) &&
                 g.back(count, s.count, (size_t)Z)
             ? 0
             : -5;
}

int mtsac_debug_act_gram(int Z, int M, int W, int ld, const float* H, double* gram, int32_t* info) {
  if (Z < 1 || Z > 64 || M < 1 || W < 1 || ld < W || !H || !gram) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t r = (size_t)act_gram_dim(M, W);
  Guarded g;
  ActGram a{};
  a.H = metrics_input(g, H, Z, M, ld);
  a.Z = Z;
  a.M = M;
  a.W = W;
  a.ld = ld;
  a.sH = (long long)M * ld;
  a.gram = g.out<double>((size_t)Z * r * r, "gram");
  a.sG = (long long)(r * r);
  if (!g.ok) return -12;
  act_gram(a, nullptr);
  int rc = 0;
  if ((rc = sync_rc("act_gram")) || (rc = g.check())) return rc;
  if (info) {
    info[0] = W <= M ? 0 : 1;
    info[1] = (int32_t)r;
  }
  return g.back(gram, a.gram, (size_t)Z * r * r) ? 0 : -5;
}

int mtsac_debug_head_backward(int form, int flags, int B, int T_l, int E, int W, int hd, const int* task, const float* h,
                              const float* Wh, const float* dout, const float* dq, float* dz, float* dbp, float* db,
                              float* planes, float* dWh, float* dbh, int* counts, int* rows, int* info) {
  const bool p3 = flags & 1, p2h = flags & 2, compact = form == 2;
  const bool hd_ok = head_kernels_cover(hd, W);  // hd 3, 5, 7 and a wide head at W % 4 != 0 have no kernel
  if (form < 0 || form > 2 || (flags & ~3) || (p3 && p2h) || !hd_ok || E < 1 || E > 4 || W < 1 || !h || !Wh || !dout ||
      !dz || !dbp || !db || !planes || !dWh || !dbh || !counts || !rows || !info || !tasks_ok(task, B, T_l) ||
      (compact && (hd != 1 || W % 4 != 0 || !dq || !(p3 || p2h))) || (long long)E * B * W >= (1LL << 28) ||
      !outputs_distinct({dz, dbp, db, planes, dWh, dbh, counts, rows, info}))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const int chunks = head_backward_chunks(T_l);
  const size_t nh = (size_t)E * B * W, nw = (size_t)E * T_l * W * hd, nd = (size_t)E * B * hd, np = p2h ? 2 : 3;
  Guarded g;
  TaskLists tl = make_lists(g, task, B, T_l);
  HeadParams hp{};
  hp.h = g.in(h, nh); hp.Wh = g.in(Wh, nw); hp.task = tl.d_task;
  hp.B = B; hp.W = W; hp.hd = hd; hp.E = E;
  hp.sWh = (long long)T_l * W * hd; hp.sbh = (long long)T_l * hd; hp.sh = (long long)B * W;
  hp.fault = g.mem.get<unsigned>(1);  // zeroed
  const float* d_dout = g.in(dout, nd);
  float* d_dz = g.out<float>(nh, "dz");
  float* d_dbp = g.out<float>((size_t)E * chunks * W, "dbp");
  float* d_db = g.out<float>((size_t)E * W, "db");
  float* d_dWh = g.out<float>(nw, "dWh");
  float* d_dbh = g.out<float>((size_t)E * T_l * hd, "dbh");
  PlaneOut po{};
  std::vector<PlaneRec> hrec(2);
  if (p3 || p2h) {
    po.p = g.out<__bf16>(np * nh, "planes");
    po.ld = W; po.ps = (long long)B * W; po.sm = (long long)np * po.ps;
  }
  if (p2h) {  // the bound's inputs: max |dout| as one partial maximum, max |head weight| in amax[1]
    std::memset(hrec.data(), 0, sizeof(PlaneRec) * 2);
    for (size_t i = 0; i < nd; ++i) hrec[0].amax[0] = std::max(hrec[0].amax[0], std::fabs(dout[i]));
    for (size_t i = 0; i < nw; ++i) hrec[1].amax[1] = std::max(hrec[1].amax[1], std::fabs(Wh[i]));
    const PlaneRec* r = g.in(hrec.data(), 2);
    po.rc = rec_out(g, 0x7fffffff, "planes rec");
    po.rd = r; po.nd = 1; po.rw = r + 1; po.w_add = 0.f; po.kmul = (float)hd;
  }
  int *d_n = nullptr, *d_slot = nullptr;
  if (compact) {
    const float* d_dq = g.in(dq, (size_t)E * B);
    d_n = g.out<int>((size_t)E, "n");
    int* d_ar = g.out<int>((size_t)E * B, "active rows");
    d_slot = g.out<int>((size_t)E * B, "slot");
    if (g.ok) active_rows(d_dq, E, B, d_n, d_ar, d_slot, nullptr);
  }
  if (!g.ok || !hp.fault) return -12;
  std::fill(info, info + 8, 0);
  const bool data = W % 4 == 0;  // the data pass's contract (kernels.h)
  if (compact) {
    head_backward_data(hp, d_dout, (long long)B * hd, nullptr, tl.counts, tl.rows, B, T_l, nullptr, po, nullptr, d_slot);
  } else if (form == 1) {
    info[0] = head_backward_both(hp, d_dout, (long long)B * hd, d_dz, tl.counts, tl.rows, B, T_l, po, d_dbp, d_dWh, d_dbh,
                                 nullptr) ? 1 : 0;
  } else {
    if (data) head_backward_data(hp, d_dout, (long long)B * hd, d_dz, tl.counts, tl.rows, B, T_l, nullptr, po, d_dbp);
    head_backward_weight(hp, d_dout, (long long)B * hd, tl.counts, tl.rows, B, d_dWh, d_dbh, nullptr);
    info[0] = data ? 1 : 0;
  }
  if (!compact && info[0]) colsum_finish(d_dbp, W, chunks, E, d_db, W, nullptr);
  int rc = 0;
  if ((rc = sync_rc("head_backward")) || (rc = g.check())) return rc;
  int ec = 0;
  if (p2h && !g.back(&ec, &po.rc->e, 1)) return -5;
  info[1] = ec;
  unsigned fault = 0;
  if (!g.back(&fault, hp.fault, 1)) return -5;
  info[2] = (int)fault;
  if (compact && !g.back(info + 3, d_n, (size_t)E)) return -5;
  if (po.p) {
    // a split2h launch that wrote no exponent leaves nothing to unscale: the planes come back as they lie (NaN)
    for (int e = 0; e < E; ++e)
      if (!planes_sum(po.p + (size_t)e * po.sm, np * (size_t)po.ps, (size_t)po.ps, (size_t)po.ps, p2h,
                      ec == 0x7fffffff ? 0 : ec, planes + (size_t)e * po.ps))
        return -5;
  }
  return g.back(dz, d_dz, nh) && g.back(dbp, d_dbp, (size_t)E * chunks * W) && g.back(db, d_db, (size_t)E * W) &&
                 g.back(dWh, d_dWh, nw) && g.back(dbh, d_dbh, (size_t)E * T_l * hd) &&
                 g.back(counts, tl.counts, (size_t)T_l) && g.back(rows, tl.rows, (size_t)T_l * B)
             ? 0
             : -5;
}

int mtsac_debug_head_action_grad(int B, int E, int Wc, int Ic, int A, const float* dz1, const float* dq, const float* W0,
                                 const float* cache, const float* alpha_w, const float* a_data, int ld_a_data,
                                 float explore_scale, float ls_min, float ls_max, const float* row_loss_in, float* dout,
                                 float* row_loss, float* row_explore, float* dout_amax, int* dout_parts) {
  if (B < 1 || E < 1 || E > 4 || Wc < 1 || A < 1 || A > 64 || (A > 8 && Wc % 4 != 0) || Ic < A || !dz1 || !W0 || !cache || !alpha_w || !dout ||
      !row_loss || !row_explore || !dout_amax || !dout_parts || (a_data && (ld_a_data < A || !row_loss_in)) ||
      (long long)E * B * Wc >= (1LL << 28) || !outputs_distinct({dout, row_loss, row_explore, dout_amax, dout_parts}))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t nz = (size_t)E * B * Wc;
  Guarded g;
  ActionGradParams p{};
  std::vector<float> zc;
  if (dq) {  // member e's active rows (dq != 0) compacted in ascending order; the rest of the buffer is NaN
    const float* d_dq = g.in(dq, (size_t)E * B);
    int* d_n = g.out<int>((size_t)E, "n");
    int* d_ar = g.out<int>((size_t)E * B, "active rows");
    int* d_slot = g.out<int>((size_t)E * B, "slot");
    if (!g.ok) return -12;
    active_rows(d_dq, E, B, d_n, d_ar, d_slot, nullptr);
    if (int rc = sync_rc("active_rows")) return rc;
    std::vector<int> hs((size_t)E * B);
    if (!g.back(hs.data(), d_slot, hs.size())) return -5;
    zc.assign(nz, std::nanf(""));
    for (size_t i = 0; i < hs.size(); ++i) {
      if (hs[i] >= B) return -5;
      if (hs[i] >= 0) std::copy(dz1 + i * Wc, dz1 + (i + 1) * Wc, zc.begin() + ((i / B) * B + hs[i]) * Wc);
    }
    p.slot = d_slot;
  }
  p.dz1 = g.in(dq ? zc.data() : dz1, nz);
  p.W0 = g.in(W0, (size_t)E * Ic * Wc);
  p.s_dz = (long long)B * Wc; p.s_W0 = (long long)Ic * Wc;
  p.E = E; p.B = B; p.Wc = Wc; p.A = A;
  p.cache = g.in(cache, (size_t)B * 5 * A);
  p.alpha_w = g.in(alpha_w, (size_t)B);
  p.ls_min = ls_min; p.ls_max = ls_max;
  p.dout = g.out<float>((size_t)B * 2 * A, "dout");
  p.dout_rec = rec_out(g, 0, "dout_rec");
  int parts = -1;
  p.dout_parts = &parts;
  p.a_data = g.in(a_data, (size_t)B * (a_data ? ld_a_data : 0));
  p.ld_a_data = ld_a_data; p.explore_scale = explore_scale;
  p.row_loss = g.out<float>((size_t)B, "row_loss");
  p.row_explore = g.out<float>((size_t)B, "row_explore");
  if (!g.ok) return -12;
  if (a_data && hipMemcpy(p.row_loss, row_loss_in, sizeof(float) * B, hipMemcpyHostToDevice) != hipSuccess) return -5;
  if (!action_grad(p, nullptr)) return -22;
  int rc = 0;
  if ((rc = sync_rc("action_grad")) || (rc = g.check())) return rc;
  *dout_parts = parts;
  return g.back(dout, p.dout, (size_t)B * 2 * A) && g.back(row_loss, p.row_loss, (size_t)B) &&
                 g.back(row_explore, p.row_explore, (size_t)B) && g.back(dout_amax, p.dout_rec->amax, (size_t)PLANE_REC_PARTS)
             ? 0
             : -5;
}

int mtsac_debug_head_row_alpha(int B, int T_l, int T_glob, int task_begin, int use_tw, const int* task,
                               const float* log_alpha, float* alpha_row, float* tw_row) {
  if (task_begin < 0 || T_glob < task_begin + T_l || !log_alpha || !alpha_row || !tw_row || !tasks_ok(task, B, T_l))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const int* d_task = g.in(task, (size_t)B);
  const float* d_la = g.in(log_alpha, (size_t)T_glob);
  float* d_a = g.out<float>((size_t)B, "alpha_row");
  float* d_tw = g.out<float>((size_t)B, "tw_row");
  if (!g.ok) return -12;
  row_alpha(d_task, task_begin, d_la, T_glob, B, use_tw != 0, d_a, d_tw, nullptr);
  int rc = 0;
  if ((rc = sync_rc("row_alpha")) || (rc = g.check())) return rc;
  return g.back(alpha_row, d_a, (size_t)B) && g.back(tw_row, d_tw, (size_t)B) ? 0 : -5;
}

// gemm_x3f / gemm_x3s as the engine's trunk calls them (mtsac_debug.h): padded plane strides, guarded
// outputs, the bias grad's column-sum partials and their finish over the engine's own chunk count
int mtsac_debug_gemm_x3f_ld(int epi, int batch, int M, int N, int K, int ld_n, int rows_p, const float* A,
                            const float* B, float* C, const float* bias, const float* mask, float* Csum, float* dbp,
                            float* db, int* info) {
  const bool m16 = (epi >> 8) & 1;
  const bool small = (epi >> 9) & 1;          // gemm_x3s instead
  const int np = ((epi >> 10) & 1) ? 1 : 3;   // bf16: the high plane only
  const bool autosplit = (epi >> 11) & 1;     // split-K by the launcher's own choice (workspace given)
  const bool fin = (epi >> 12) & 1;           // ... with arrival counters: the in-launch finish
  const bool h2 = (epi >> 13) & 1;            // precision split2h
  const bool bfrag = (epi >> 14) & 1;         // B planes in the fragment layout (N % 16 == 0)
  const bool ponly = (epi >> 15) & 1;         // planes only: the engine's data-grad form
  epi &= 255;
  if (M < 1 || N < 1 || K < 1 || batch < 1 || batch > 8 || ld_n < N || ld_n % 4 != 0 || rows_p < M || !A || !B ||
      !Csum || !dbp || !db || !info || (!ponly && !C) || (epi != EPI_BIAS_RELU && epi != EPI_RELU_MASK) ||
      (epi == EPI_BIAS_RELU && !bias) || (epi == EPI_RELU_MASK && !mask) || (bfrag && N % 16 != 0) ||
      (h2 && np == 1) || (long long)batch * rows_p * ld_n >= (1LL << 28))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const long long Kp = small ? up32(K) : (K + 63) / 64 * 64;  // gemm_x3s steps K by 32 (the engine's padded width)
  const size_t nA = (size_t)M * K * batch, nB = (size_t)N * K * batch, nC = (size_t)M * N * batch;
  const long long pp = (long long)rows_p * ld_n;  // plane stride of the output and mask planes
  const int maxrt = gemm_x3f_max_row_tiles(M);
  Guarded gd;
  std::vector<PlaneRec> hrec(4);
  std::memset(hrec.data(), 0, sizeof(PlaneRec) * 4);
  if (h2) {  // records of A, B (its max covering the bias, as a trunk record does), the mask and C
    const float ma = host_amax(A, nA), mbias = epi == EPI_BIAS_RELU ? host_amax(bias, (size_t)N * batch) : 0.f;
    const float mb = std::max(host_amax(B, nB), mbias), mm = mask ? host_amax(mask, nC) : 1.f;
    hrec[0].e = host_plane_exp(ma); hrec[0].amax[0] = ma;
    hrec[1].e = host_plane_exp(mb); hrec[1].amax[0] = mb;
    hrec[2].e = host_plane_exp(mm); hrec[2].amax[0] = mm;
  }
  PlaneRec* rec = gd.in(hrec.data(), 4);
  const float *dA = gd.in(A, nA), *dB = gd.in(B, nB), *dbias = gd.in(bias, (size_t)N * batch), *dmask = gd.in(mask, nC);
  __bf16* Ap = gd.mem.get<__bf16>((size_t)3 * rows_p * Kp * batch);
  __bf16* Bp = gd.mem.get<__bf16>((size_t)3 * N * Kp * batch);
  __bf16* Mp = m16 ? gd.mem.get<__bf16>((size_t)3 * pp * batch) : nullptr;
  float* dC = ponly ? nullptr : gd.out<float>(nC, "C");
  __bf16* dCp = gd.out<__bf16>((size_t)3 * pp * batch, "C planes");
  float* d_dbp = gd.out<float>((size_t)batch * maxrt * N, "dbp");
  float* d_db = gd.out<float>((size_t)batch * N, "db");
  if (!gd.ok || !rec || !Ap || !Bp || (m16 && !Mp)) return -12;
  SplitGemmParams g{};
  g.A = Ap; g.lda = Kp; g.pA = (long long)rows_p * Kp; g.sA = 3 * g.pA;
  g.B = Bp; g.ldb = Kp; g.pB = (long long)N * Kp; g.sB = 3 * g.pB;
  g.b_frag = bfrag ? 1 : 0;
  g.C = dC; g.ldc = N; g.sC = (long long)M * N;
  g.bias = dbias; g.sBias = N;
  if (m16) {
    g.mask16 = Mp; g.ldm = ld_n; g.sMask = 3 * pp;
  } else {
    g.mask = dmask; g.ldm = N; g.sMask = (long long)M * N;
  }
  g.pMask = pp;
  g.Cp = dCp; g.ldcp = ld_n; g.pC = pp; g.sCp = 3 * pp;
  g.M = M; g.N = N; g.K = (int)Kp;
  g.np = h2 ? 2 : np;
  g.dbp = d_dbp;
  int nparts = 0;
  g.nparts = &nparts;
  if (h2) {
    g.ra = rec + 0; g.na = 1;
    g.rb = rec + 1; g.nb = 1;
    g.rc = rec + 3;
    g.bias_in_b = epi == EPI_BIAS_RELU ? 1 : 0;
    g.kmul = (float)K;
  }
  if (autosplit) {
    g.ws = gd.mem.get<float>((size_t)std::max(gemm_x3f_ws_floats(M, N, (int)Kp, batch), 1LL));
    if (!g.ws) return -12;
    g.splits = -1;
    if (fin && !(g.cnt = gd.mem.get<int>((size_t)GEMM_X3F_CNT))) return -12;  // zeroed
  }
  if (small ? !gemm_x3s_ok(g, epi, batch) : !gemm_x3f_ok(g, epi, batch)) return -95;
  // rows per column-sum chunk and the chunk count, by the rule the engine's dgrad_params uses
  const int bm = dbp_chunk_rows(g, epi, batch, !small);
  const int chunks = (M + bm - 1) / bm;
  if (chunks > maxrt) return -95;
  for (int z = 0; z < batch; ++z) {
    SplitParams s{};
    s.x = dA + (size_t)z * M * K; s.ldx = K; s.rows = M; s.cols = K;
    s.out = Ap + (size_t)z * 3 * rows_p * Kp; s.ldo = Kp; s.po = (long long)rows_p * Kp; s.out_rows = rows_p;
    s.out_cols = (int)Kp;
    s.e2h = h2 ? &rec[0].e : nullptr;
    split_planes(s, false, 1, nullptr);  // zero rows past M, zero columns past K
    s.x = dB + (size_t)z * N * K; s.rows = N;
    s.out = Bp + (size_t)z * 3 * N * Kp; s.po = (long long)N * Kp; s.out_rows = N;
    s.e2h = h2 ? &rec[1].e : nullptr;
    s.frag = bfrag ? 1 : 0;
    split_planes(s, false, 1, nullptr);
    s.frag = 0;
    if (m16) {  // planes of the mask, row stride ld_n, rows_p rows per plane (zeros in the padding)
      s.x = dmask + (size_t)z * M * N; s.ldx = N; s.rows = M; s.cols = N;
      s.out = Mp + (size_t)z * 3 * pp; s.ldo = ld_n; s.po = pp; s.out_rows = rows_p; s.out_cols = ld_n;
      s.e2h = h2 ? &rec[2].e : nullptr;
      split_planes(s, false, 1, nullptr);
    }
  }
  int rc = 0;
  if ((rc = sync_rc("split_planes"))) return rc;
  int slices = 1;
  if (small) gemm_x3s(g, epi, batch, nullptr);
  else slices = gemm_x3f(g, epi, batch, nullptr);
  colsum_finish(d_dbp, N, chunks, batch, d_db, N, nullptr);
  if ((rc = sync_rc(small ? "gemm_x3s" : "gemm_x3f")) || (rc = gd.check())) return rc;
  int ec = 0;
  if (h2 && !gd.back(&ec, &rec[3].e, 1)) return -5;
  // split launches: the in-launch finish keeps the split row tile, the finishing pass sums shorter chunks
  info[0] = small ? 3 : slices <= 1 ? 0 : bm == gemm_x3f_split_bm(M, N, (int)Kp, batch) ? 1 : 2;
  info[1] = bm;
  info[2] = chunks;
  info[3] = slices;
  info[4] = nparts;
  info[5] = maxrt;
  info[6] = ec;
  info[7] = small ? gemm_x3s_ti(M, N, batch) : slices > 1 ? gemm_x3f_split_bm(M, N, (int)Kp, batch) : gemm_x3f_bm(g, batch);
  if (dC && !gd.back(C, dC, nC)) return -5;
  // bf16 keeps the high plane only (gemm_x3f leaves the other two alone)
  const size_t per = (size_t)pp;
  for (int z = 0; z < batch; ++z) {
    if (np == 1 && !h2) {
      std::vector<__bf16> h(per);
      if (hipMemcpy(h.data(), dCp + (size_t)z * 3 * per, per * 2, hipMemcpyDeviceToHost) != hipSuccess) return -5;
      for (size_t i = 0; i < per; ++i) Csum[(size_t)z * per + i] = (float)h[i];
    } else if (!planes_sum(dCp + (size_t)z * 3 * per, 3 * per, per, per, h2, ec, Csum + (size_t)z * per)) {
      return -5;
    }
  }
  return gd.back(dbp, d_dbp, (size_t)batch * maxrt * N) && gd.back(db, d_db, (size_t)batch * N) ? 0 : -5;
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
  long long lda, pa, ldb, pb;
  plane_geom(M, K, true, lda, pa);
  plane_geom(N, K, true, ldb, pb);
  Guarded gd;
  const float *dA = gd.in(A, (size_t)E * K * M), *dB = gd.in(B, (size_t)E * K * N);
  const float* dpart = gd.in(part, (size_t)E * chunks * N);
  __bf16* Ap = gd.mem.get<__bf16>((size_t)3 * pa * E);
  __bf16* Bp = gd.mem.get<__bf16>((size_t)3 * pb * E);
  float* dC = gd.out<float>((size_t)E * M * N, "C");
  float* d_db = gd.out<float>((size_t)E * N, "db");
  const int want = splits == 0 ? gemm_x3p_splits(M, N, Kp, E, true, 3) : splits;
  float* ws = gd.mem.get<float>((size_t)std::max(gemm_ws_floats(M, N, E, std::max(want, 2)), 1LL));
  if (!gd.ok || !Ap || !Bp || !ws) return -12;
  const float *dpre = nullptr, *dpost = nullptr;
  float *d_dbpre = nullptr, *d_dbpost = nullptr;
  if (mode == 1) {
    dpre = gd.in(part_pre, (size_t)E * nb[0] * nb[1]);
    dpost = gd.in(part_post, (size_t)E * nb[2] * nb[3]);
    d_dbpre = gd.out<float>((size_t)E * nb[1], "db_pre");
    d_dbpost = gd.out<float>((size_t)E * nb[3], "db_post");
    if (!gd.ok) return -12;
  }
  for (int z = 0; z < E; ++z) {
    split_into(dA + (size_t)z * K * M, M, K, true, Ap + 3 * pa * z);
    split_into(dB + (size_t)z * K * N, N, K, true, Bp + 3 * pb * z);
  }
  SplitGemmParams g{};
  g.A = Ap; g.lda = lda; g.pA = pa; g.sA = 3 * pa; g.a_kmajor = 1;
  g.B = Bp; g.ldb = ldb; g.pB = pb; g.sB = 3 * pb; g.b_kmajor = 1;
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

// the layout kernels alone (mtsac_debug.h): split_planes, transpose_f32, colsum
int mtsac_debug_layout(int kind, const int* dims, const float* x, void* out, void* out2) {
  if (kind < 0 || kind > 2 || !dims || !x || !out) return -22;
  if (kind == 0) {
    const int rows = dims[0], cols = dims[1], ldx = dims[2], out_rows = dims[3], out_cols = dims[4], ldo = dims[5],
              arows = dims[6], tr = dims[7], batch = dims[8], frag = dims[9], h2 = dims[10], e = dims[11];
    if (rows < 1 || cols < 1 || ldx < cols || out_rows < 1 || out_cols < 1 || ldo < out_cols || arows < out_rows ||
        (tr & ~1) || batch < 1 || batch > 8 || (frag & ~1) || (h2 & ~1) || e < -100 || e > 100 ||
        (frag && (ldo % 32 != 0 || arows % 16 != 0)) || (long long)batch * arows * ldo >= (1LL << 27) ||
        (long long)batch * rows * ldx >= (1LL << 27))
      return -22;
    if (hipSetDevice(0) != hipSuccess) return -5;
    Guarded gd;
    const long long po = (long long)arows * ldo;
    const float* dx = gd.in(x, (size_t)batch * rows * ldx);
    const int* de = gd.in(&e, 1);
    __bf16* dout = gd.out<__bf16>((size_t)batch * 3 * po, "planes");
    if (!gd.ok) return -12;
    SplitParams s{};
    s.x = dx; s.ldx = ldx; s.sx = (long long)rows * ldx; s.rows = rows; s.cols = cols;
    s.out = dout; s.ldo = ldo; s.po = po; s.so = 3 * po; s.out_rows = out_rows; s.out_cols = out_cols;
    s.e2h = h2 ? de : nullptr;
    s.frag = frag;
    split_planes(s, tr != 0, batch, nullptr);
    int rc = 0;
    if ((rc = sync_rc("split_planes")) || (rc = gd.check())) return rc;
    return gd.back(reinterpret_cast<__bf16*>(out), dout, (size_t)batch * 3 * po) ? 0 : -5;
  }
  if (kind == 1) {
    const int rows = dims[0], cols = dims[1], batch = dims[2];
    if (rows < 1 || cols < 1 || batch < 1 || batch > 8 || (long long)batch * rows * cols >= (1LL << 27)) return -22;
    if (hipSetDevice(0) != hipSuccess) return -5;
    Guarded gd;
    const size_t n = (size_t)rows * cols;
    const float* dx = gd.in(x, n * batch);
    float* dout = gd.out<float>(n * batch, "transposed");
    if (!gd.ok) return -12;
    transpose_f32(dx, (long long)n, dout, (long long)n, rows, cols, batch, nullptr);
    int rc = 0;
    if ((rc = sync_rc("transpose_f32")) || (rc = gd.check())) return rc;
    return gd.back(reinterpret_cast<float*>(out), dout, n * batch) ? 0 : -5;
  }
  const int rows = dims[0], cols = dims[1], ld = dims[2], batch = dims[3];
  if (rows < 1 || cols < 1 || ld < cols || batch < 1 || batch > 8 || !out2 ||
      (long long)batch * rows * ld >= (1LL << 27))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded gd;
  const float* dx = gd.in(x, (size_t)batch * rows * ld);
  float* dpart = gd.out<float>((size_t)batch * COLSUM_CHUNKS * cols, "part");
  float* d_db = gd.out<float>((size_t)batch * cols, "db");
  if (!gd.ok) return -12;
  colsum(dx, rows, cols, ld, (long long)rows * ld, batch, dpart, d_db, cols, nullptr);
  int rc = 0;
  if ((rc = sync_rc("colsum")) || (rc = gd.check())) return rc;
  return gd.back(reinterpret_cast<float*>(out), dpart, (size_t)batch * COLSUM_CHUNKS * cols) &&
                 gd.back(reinterpret_cast<float*>(out2), d_db, (size_t)batch * cols)
             ? 0
             : -5;
}

// ---- the replay kernels (replay.hip) ----
extern int pcg_jump_table(unsigned long long* out);  // engine.cpp: 65 x (A_hi, A_lo, C_hi, C_lo)

int mtsac_debug_replay_indices(uint64_t* state, int mode, int64_t high_or_size, int n, int n_alloc, int32_t* idx) {
  if (!state || !idx || (mode != 0 && mode != 1) || n < 1 || n_alloc < n || n_alloc > (1 << 24) || high_or_size < 1 ||
      high_or_size >= (1LL << 31) || (state[4] & ~1ull) || state[5] > 0xFFFFFFFFull)
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  unsigned long long jt[65 * 4];
  pcg_jump_table(jt);
  PcgDev s{state[0], state[1], state[2], state[3], (int)state[4], (unsigned)state[5]};
  const long long size = high_or_size;
  Guarded g;
  const unsigned long long* d_jump = g.in(jt, (size_t)65 * 4);
  const long long* d_size = g.in(&size, 1);
  PcgDev* d_rng = guarded_inout(g, &s, 1, "rng");
  int* d_idx = g.out<int>((size_t)n_alloc, "idx");
  if (!g.ok) return -12;
  if (mode == 0) replay_indices_high(d_rng, d_jump, size, n, d_idx, nullptr);
  else replay_indices(d_rng, d_jump, d_size, n, d_idx, nullptr);
  int rc = 0;
  if ((rc = sync_rc("replay_indices")) || (rc = g.check())) return rc;
  if (!g.back(&s, d_rng, 1) || !g.back(idx, d_idx, (size_t)n_alloc)) return -5;
  state[0] = s.state_hi; state[1] = s.state_lo; state[2] = s.inc_hi; state[3] = s.inc_lo;
  state[4] = (uint64_t)(unsigned)s.has_uint32; state[5] = s.uinteger;
  return 0;
}

int mtsac_debug_replay_gather(const int* dims, const float* store, const int32_t* idx, const float* u_obs,
                              const float* u_act, const float* u_nobs, const float* u_done, const float* u_rew,
                              const double* rmin, const double* rmax, double norm_eps, const float* in_max, float* xa,
                              float* xa_next, float* xc, float* xc_next, float* xc_pi, float* rew, float* done,
                              int32_t* task, int32_t* err, uint16_t* pa, uint16_t* pc, uint16_t* pcn, uint16_t* pcp,
                              int32_t* in_rec_e) {
  if (!dims) return -22;
  const int src = dims[0], n = dims[1], T_l = dims[2], cap = dims[3], D = dims[4], A = dims[5], T_glob = dims[6],
            task_begin = dims[7], ld_a = dims[8], ld_c = dims[9], pm = dims[10], pa_ld = dims[11], pc_ld = dims[12],
            pa_next = dims[13], pa_rows = dims[14], pc_rows = dims[15], R = dims[16];
  if ((src != 0 && src != 1) || n < 1 || T_l < 1 || T_l > 64 || D < 1 || A < 1 || A > 64 || T_glob < 1 || T_glob > D ||
      task_begin < 0 || ld_a < D || ld_c < A + D || R < 2 * D + A + 2 || pm < 0 || pm > 2 || (long long)n * T_l > (1 << 20) ||
      !xa || !xa_next || !xc || !xc_next || !xc_pi || !rew || !done || !task || !err || (rmin == nullptr) != (rmax == nullptr))
    return -22;
  const int B = src == 0 ? n * T_l : n;
  if (src == 0) {
    if (!store || !idx || cap < 1 || (long long)cap * T_l * R >= (1LL << 27)) return -22;
    for (int i = 0; i < n; ++i)
      if (idx[i] < 0 || idx[i] >= cap) return -22;
  } else if (!u_obs || !u_act || !u_nobs || !u_done || !u_rew) {
    return -22;
  }
  if (pm && (!pa || !pc || !pcn || !pcp || pa_ld < D || pc_ld < A + D || pa_next < 0 || pa_rows < pa_next + B || pc_rows < B ||
             (pm == 2 && (!in_max || !in_rec_e))))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  GatherParams p{};
  p.store = src == 0 ? g.in(store, (size_t)cap * T_l * R) : nullptr;
  p.idx = src == 0 ? g.in(idx, (size_t)n) : nullptr;
  p.n = n; p.T_l = T_l; p.R = R; p.obs_dim = D; p.act_dim = A; p.T_glob = T_glob; p.task_begin = task_begin;
  p.ld_a = ld_a; p.ld_c = ld_c;
  p.xa = g.out<float>((size_t)B * ld_a, "xa");
  p.xa_next = g.out<float>((size_t)B * ld_a, "xa_next");
  p.xc = g.out<float>((size_t)B * ld_c, "xc");
  p.xc_next = g.out<float>((size_t)B * ld_c, "xc_next");
  p.xc_pi = g.out<float>((size_t)B * ld_c, "xc_pi");
  p.rew = g.out<float>((size_t)B, "rew");
  p.done = g.out<float>((size_t)B, "done");
  p.task = g.out<int>((size_t)B, "task");
  p.err = g.out<int>(1, "err");
  if (p.err && hipMemset(p.err, 0, sizeof(int)) != hipSuccess) g.ok = false;
  p.rmin = g.in(rmin, (size_t)T_l);
  p.rmax = g.in(rmax, (size_t)T_l);
  p.norm_eps = norm_eps;
  const int np = pm == 2 ? 2 : 3;
  const size_t pa_ps = (size_t)pa_rows * pa_ld, pc_ps = (size_t)pc_rows * pc_ld;
  PlaneRec* rec = nullptr;
  if (pm) {
    p.pa = g.out<__bf16>(np * pa_ps, "pa");
    p.pc = g.out<__bf16>(np * pc_ps, "pc");
    p.pcn = g.out<__bf16>(np * pc_ps, "pcn");
    p.pcp = g.out<__bf16>(np * pc_ps, "pcp");
    p.pa_ps = (long long)pa_ps; p.pa_next = pa_next; p.pa_ld = pa_ld; p.pc_ps = (long long)pc_ps; p.pc_ld = pc_ld;
    if (pm == 2) {
      rec = g.out<PlaneRec>(1, "in_rec");
      p.in_rec = rec;
      p.in_max = g.in(in_max, 1);
    }
  }
  const float *d_o = nullptr, *d_a = nullptr, *d_no = nullptr, *d_d = nullptr, *d_r = nullptr;
  if (src == 1) {
    d_o = g.in(u_obs, (size_t)B * D); d_a = g.in(u_act, (size_t)B * A); d_no = g.in(u_nobs, (size_t)B * D);
    d_d = g.in(u_done, (size_t)B); d_r = g.in(u_rew, (size_t)B);
  }
  if (!g.ok) return -12;
  if (src == 0) replay_gather(p, nullptr);
  else batch_scatter(p, d_o, d_a, d_no, d_d, d_r, B, nullptr);
  int rc = 0;
  if ((rc = sync_rc("gather")) || (rc = g.check())) return rc;
  bool ok = g.back(xa, p.xa, (size_t)B * ld_a) && g.back(xa_next, p.xa_next, (size_t)B * ld_a) &&
            g.back(xc, p.xc, (size_t)B * ld_c) && g.back(xc_next, p.xc_next, (size_t)B * ld_c) &&
            g.back(xc_pi, p.xc_pi, (size_t)B * ld_c) && g.back(rew, p.rew, (size_t)B) && g.back(done, p.done, (size_t)B) &&
            g.back(task, p.task, (size_t)B) && g.back(err, p.err, 1);
  if (ok && pm)
    ok = g.back(reinterpret_cast<__bf16*>(pa), p.pa, np * pa_ps) && g.back(reinterpret_cast<__bf16*>(pc), p.pc, np * pc_ps) &&
         g.back(reinterpret_cast<__bf16*>(pcn), p.pcn, np * pc_ps) && g.back(reinterpret_cast<__bf16*>(pcp), p.pcp, np * pc_ps);
  if (ok && rec) ok = g.back(in_rec_e, &rec->e, 1);
  return ok ? 0 : -5;
}

int mtsac_debug_task_rows(int B, int T_l, int max_rows, const int32_t* task, int32_t* counts, int32_t* rows) {
  if (!tasks_ok(task, B, T_l) || max_rows < 1 || !counts || !rows || (long long)T_l * max_rows > (1 << 24)) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const int* d_task = g.in(task, (size_t)B);
  int* d_counts = g.out<int>((size_t)T_l, "counts");
  int* d_rows = g.out<int>((size_t)T_l * max_rows, "rows");
  if (!g.ok) return -12;
  task_rows(d_task, B, T_l, d_counts, d_rows, max_rows, nullptr);
  int rc = 0;
  if ((rc = sync_rc("task_rows")) || (rc = g.check())) return rc;
  return g.back(counts, d_counts, (size_t)T_l) && g.back(rows, d_rows, (size_t)T_l * max_rows) ? 0 : -5;
}

int mtsac_debug_pack_commit(int T_l, int D, int A, int R, int64_t size, const float* obs, const float* nobs,
                            const float* act, const float* rew, const float* done, float* rec, double* rmin,
                            double* rmax, int64_t* buf_size, float* bufmax) {
  if (T_l < 1 || T_l > 64 || D < 1 || A < 1 || R < 2 * D + A + 2 || (long long)T_l * R > (1 << 24) || !obs || !nobs || !act ||
      !rew || !done || !rec || !buf_size || (rmin == nullptr) != (rmax == nullptr))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const float *d_o = g.in(obs, (size_t)T_l * D), *d_no = g.in(nobs, (size_t)T_l * D), *d_a = g.in(act, (size_t)T_l * A);
  const float *d_r = g.in(rew, (size_t)T_l), *d_d = g.in(done, (size_t)T_l);
  float* d_rec = g.out<float>((size_t)T_l * R, "rec");
  double* d_min = rmin ? guarded_inout(g, rmin, (size_t)T_l, "rmin") : nullptr;
  double* d_max = rmax ? guarded_inout(g, rmax, (size_t)T_l, "rmax") : nullptr;
  long long* d_size = g.out<long long>(1, "buf_size");
  float* d_bm = bufmax ? guarded_inout(g, bufmax, 1, "bufmax") : nullptr;
  if (!g.ok) return -12;
  buffer_pack_slot(d_rec, T_l, R, D, A, d_o, d_no, d_a, d_r, d_d, nullptr);
  buffer_commit_slot(d_rec, T_l, R, D + A, d_min, d_max, d_size, (long long)size, nullptr, D, d_bm);
  int rc = 0;
  if ((rc = sync_rc("pack / commit slot")) || (rc = g.check())) return rc;
  long long sz = 0;
  bool ok = g.back(rec, d_rec, (size_t)T_l * R) && g.back(&sz, d_size, 1);
  *buf_size = sz;
  if (ok && rmin) ok = g.back(rmin, d_min, (size_t)T_l) && g.back(rmax, d_max, (size_t)T_l);
  if (ok && bufmax) ok = g.back(bufmax, d_bm, 1);
  return ok ? 0 : -5;
}

int mtsac_debug_absmax(int64_t n, const float* x, float* m) {
  if (n < 1 || n > (1 << 26) || !x || !m) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const float* d_x = g.in(x, (size_t)n);
  float* d_m = guarded_inout(g, m, 1, "m");
  if (!g.ok) return -12;
  absmax_into(d_x, (long long)n, d_m, nullptr);
  int rc = 0;
  if ((rc = sync_rc("absmax_into")) || (rc = g.check())) return rc;
  return g.back(m, d_m, 1) ? 0 : -5;
}

int mtsac_debug_fill_synthetic(int64_t cap, int T_l, int D, int A, int T_glob, int task_begin, uint64_t seed,
                               float* store, float* bufmax) {
  if (cap < 1 || T_l < 1 || D < 1 || A < 1 || T_glob < 1 || T_glob > D || task_begin < 0 || task_begin + T_l > T_glob ||
      !store || !bufmax)
    return -22;
  const int R = (2 * D + A + 2 + 3) / 4 * 4;
  if ((long long)cap * T_l * R > (1 << 26)) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  Guarded g;
  const size_t nf = (size_t)cap * T_l * R;
  float* d_store = g.out<float>(nf, "store");
  float* d_bm = guarded_inout(g, bufmax, 1, "bufmax");
  if (!g.ok) return -12;
  fill_synthetic(d_store, (long long)cap, T_l, R, D, A, T_glob, task_begin, seed, nullptr, d_bm);
  int rc = 0;
  if ((rc = sync_rc("fill_synthetic")) || (rc = g.check())) return rc;
  return g.back(store, d_store, nf) && g.back(bufmax, d_bm, 1) ? 0 : -5;
}

}  // extern "C"
