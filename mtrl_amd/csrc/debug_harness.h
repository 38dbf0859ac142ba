// debug_harness.h -- what the test-only entry points (debug.cpp, debug_gemm.cpp) share: device buffers with
// guard bands, plane operands built from fp32 matrices, split2h records, plane read-back, launch timing.
// Internal to those two files: everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "kernels.h"

namespace {

long long up8(long long x) { return (x + 7) / 8 * 8; }
long long up32(long long x) { return (x + 31) / 32 * 32; }

// zeroed device allocations, freed with the object
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

// Device buffers of one entry-point call.  An output lies between two 256-byte bands of GUARD_BYTE and
// starts as all-ones words (NaN as float, -1 as int, 255 as byte), so a store outside it and an element
// the kernel left alone both show; the bands only detect.
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
  T* zeros(size_t n) {  // scratch, or an output of the older entries: zeroed, no bands
    T* d = mem.get<T>(n);
    if (!d) ok = false;
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
          mtsac::set_last_error(msg);
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
  mtsac::set_last_error((std::string(what) + ": " + hipGetErrorString(e1 != hipSuccess ? e1 : e2)).c_str());
  return -5;
}

// host output buffers of one call must not share a start address: each is copied back over whatever the
// one before it left there, so the caller would read one output under another's name (null entries skipped)
bool outputs_distinct(std::initializer_list<const void*> outs) {
  for (auto a = outs.begin(); a != outs.end(); ++a)
    for (auto b = a + 1; b != outs.end(); ++b)
      if (*a != nullptr && *a == *b) return false;
  return true;
}

// ---- plane operands
// The planes of one batch entry's fp32 matrix of `rows` vectors of length K, split in its stored orientation:
// row-major [rows][K] into [3][rows_p][ld], k-major [K][rows] into [3][K padded][up8(rows)]; zeros in the padding.
struct PlaneGeom {
  bool kmajor = false;
  int kpad = 32;             // K padded to a multiple of this (32 or 64)
  int rows_p = 0;            // row-major: rows per plane (0: rows)
  long long ld = 0;          // row-major: row stride (0: the padded K)
  bool frag = false;         // fragment layout (row-major; ld % 32 == 0, rows_p % 16 == 0)
  const int* e2h = nullptr;  // split2h: the device exponent (&PlaneRec::e); null: split3
  PlaneGeom(bool kmajor_ = false, const int* e2h_ = nullptr) : kmajor(kmajor_), e2h(e2h_) {}
};
struct PlaneOp {
  __bf16* p = nullptr;               // null: the allocation failed
  long long ld = 0, ps = 0, sb = 0;  // row stride, plane stride, batch stride
  int batch = 0, rows = 0, K = 0;
  PlaneGeom g;
};

void plane_geom(int rows, int K, const PlaneGeom& g, long long& ld, long long& ps) {
  const long long Kp = (K + g.kpad - 1) / g.kpad * g.kpad;
  ld = g.kmajor ? up8(rows) : g.ld ? g.ld : Kp;
  ps = (g.kmajor ? Kp : (long long)(g.rows_p ? g.rows_p : rows)) * ld;
}

void split_into(const float* dsrc, int rows, int K, const PlaneGeom& g, __bf16* out) {
  long long ld, ps;
  plane_geom(rows, K, g, ld, ps);
  mtsac::SplitParams s{};
  s.x = dsrc;
  s.ldx = g.kmajor ? rows : K;
  s.rows = g.kmajor ? K : rows;
  s.cols = g.kmajor ? rows : K;
  s.out = out;
  s.ldo = ld;
  s.po = ps;
  s.out_rows = (int)(ps / ld);
  s.out_cols = (int)ld;
  s.e2h = g.e2h;
  s.frag = g.frag ? 1 : 0;
  mtsac::split_planes(s, false, 1, nullptr);
}

// The planes of `batch` such matrices in two steps, so that an entry can fill and check its launch parameters
// before anything runs: plane_alloc gives the strides and the zeroed planes, plane_split launches split_planes
// on matrices src_stride floats apart (0: every entry gets its own planes of the same matrix).
PlaneOp plane_alloc(DevBuf& mem, int batch, int rows, int K, const PlaneGeom& g) {
  PlaneOp o;
  plane_geom(rows, K, g, o.ld, o.ps);
  o.sb = 3 * o.ps;
  o.batch = batch; o.rows = rows; o.K = K;
  o.g = g;
  o.p = mem.get<__bf16>((size_t)o.sb * batch);
  return o;
}
void plane_split(const PlaneOp& o, const float* dsrc, long long src_stride) {
  for (int z = 0; z < o.batch; ++z) split_into(dsrc + (size_t)z * src_stride, o.rows, o.K, o.g, o.p + o.sb * z);
}
PlaneOp plane_operand(DevBuf& mem, const float* dsrc, long long src_stride, int batch, int rows, int K,
                      const PlaneGeom& g) {
  const PlaneOp o = plane_alloc(mem, batch, rows, K, g);
  if (o.p) plane_split(o, dsrc, src_stride);
  return o;
}

// the unscaled sum of n elements' planes (16-bit words, plane stride ps): split3 h + m + l, split2h
// (h + l) 2^-e, high_only (bf16, which leaves the other planes alone) h
bool planes_sum(const __bf16* dev, size_t n_words, size_t ps, size_t n, bool h2, int e, float* out,
                bool high_only = false) {
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
      if (high_only) {
        out[i] = (float)a;
        continue;
      }
      std::memcpy(&b, &w[ps + i], 2);
      std::memcpy(&c, &w[2 * ps + i], 2);
      out[i] = ((float)a + (float)b) + (float)c;
    }
  }
  return true;
}

// ---- split2h records
float host_amax(const float* x, size_t n) {
  float m = 0.f;
  for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(x[i]));
  return m;
}
// the device's plane_exp (gemm_common.h) on the host: the plane exponent of the bound b
int host_plane_exp(float b) {
  b *= 1.00390625f;
  if (!(b > 0.f) || !(b < 3.0e38f)) return 0;
  int ex;
  (void)std::frexp(b, &ex);  // b < 2^ex
  return std::min(100, std::max(-100, 15 - ex));
}
// Records as producers leave them, one per maximum (e = host_plane_exp, amax[0] = the maximum), then n_out
// output records with e = out_e and every partial maximum out_amax (zeros; or poison, so a stale slot shows).
std::vector<mtsac::PlaneRec> host_recs(std::initializer_list<float> maxima, int n_out = 0, int out_e = 0,
                                float out_amax = 0.f) {
  std::vector<mtsac::PlaneRec> r(maxima.size() + n_out);
  std::memset(r.data(), 0, sizeof(mtsac::PlaneRec) * r.size());
  size_t i = 0;
  for (float m : maxima) {
    r[i].e = host_plane_exp(m);
    r[i++].amax[0] = m;
  }
  for (; i < r.size(); ++i) {
    r[i].e = out_e;
    std::fill(r[i].amax, r[i].amax + mtsac::PLANE_REC_PARTS, out_amax);
  }
  return r;
}

// ---- timing entries
// one warm-up call of fn, then iters calls between two events: *ms_per_call, or the first HIP error
template <typename F>
hipError_t time_launches(int iters, F&& fn, double* ms_per_call) {
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  fn();
  hipError_t e = hipEventCreate(&ev.a);
  if (e == hipSuccess) e = hipEventCreate(&ev.b);
  if (e == hipSuccess) e = hipEventRecord(ev.a, nullptr);
  for (int i = 0; e == hipSuccess && i < iters; ++i) fn();
  if (e == hipSuccess) e = hipEventRecord(ev.b, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(ev.b);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev.a, ev.b);
  if (e == hipSuccess) *ms_per_call = ms / iters;
  return e;
}

// ---- the flag bits 8..15 that the gemm_x3f entries and the forward bench pass above the epilogue in `epi`
struct EpiFlags {
  int epi;         // the epilogue itself (low byte)
  bool m16;        // 8: ReLU mask from its bf16 / fp16 planes instead of the fp32 mask
  bool small;      // 9: gemm_x3s instead of gemm_x3f
  bool bf16;       // 10: the high plane only
  bool autosplit;  // 11: split-K by the launcher's own choice (workspace given)
  bool fin;        // 12: ... with arrival counters: the in-launch finish
  bool h2;         // 13: precision split2h, fp16 planes scaled per tensor
  bool bfrag;      // 14: B planes in the fragment layout (N % 16 == 0)
  bool ponly;      // 15: planes only, the engine's data-grad form
  explicit EpiFlags(int e)
      : epi(e & 255), m16((e >> 8) & 1), small((e >> 9) & 1), bf16((e >> 10) & 1), autosplit((e >> 11) & 1),
        fin((e >> 12) & 1), h2((e >> 13) & 1), bfrag((e >> 14) & 1), ponly((e >> 15) & 1) {}
  int np() const { return h2 ? 2 : bf16 ? 1 : 3; }  // operand planes
};

}  // namespace
