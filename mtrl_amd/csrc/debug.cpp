// debug.cpp -- test-only entry points (include/mtsac_debug.h): the DrQ kernels, the SAC heads, the layout and
// replay kernels, on debug_harness.h.  The GEMMs' entry points are in debug_gemm.cpp.
#include "../../include/mtsac.h"
#include "../../include/mtsac_debug.h"
#include "debug_harness.h"
#include "drq_kernels.h"

using namespace mtsac;

namespace {

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

}  // namespace

extern "C" {

// The DrQ conv switches (drq::ConvSwitches, meanings in mtsac_debug.h).  drq::conv_plan reads them
// when an engine is created and when a debug conv entry point is called; an engine that exists
// keeps its plans.  Each setter returns the previous value.
int mtsac_debug_drq_groups(int fwd, int bwd) {
  drq::ConvSwitches& sw = drq::conv_switches();
  const int old = sw.fwd_g | (sw.bwd_g << 8);
  sw.fwd_g = fwd;
  sw.bwd_g = bwd;
  return old;
}
int mtsac_debug_drq_legacy(int mask) {  // < 0: query only
  const int old = drq::conv_switches().legacy;
  if (mask >= 0) drq::conv_switches().legacy = mask & 63;
  return old;
}
int mtsac_debug_drq_wgrad_blocks(int cap) {  // 0: the per-shape default; < 0: query only
  const int old = drq::conv_switches().wg_blocks;
  if (cap >= 0) drq::conv_switches().wg_blocks = cap;
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

// the plan of a conv of `kind` at this shape under the current switches (drq::conv_plan)
int mtsac_debug_drq_conv_path(int kind, int B, int H, int W, int ci, int co, int* out) {
  if (kind < 0 || kind > 2 || B < 1 || H < 1 || W < 1 || !out || !drq::conv_supported(ci, co) ||
      (long long)B * H * W * 16 >= (1LL << 31))
    return -22;
  const drq::ConvPlan p = drq::conv_plan(kind, B, H, W, ci, co);
  const bool tiled = p.family != 0;
  out[0] = p.family;
  out[1] = !tiled ? 0 : kind == 2 ? p.wg.R : p.geo.R;
  out[2] = !tiled ? 0 : kind == 2 ? p.wg.tiles / B : p.geo.n;
  out[3] = drq::conv_blocks(p, B);
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
  const drq::ConvPlan pl = drq::conv_plan(kind, B, H, W, ci, co);  // sizes and launches below: this one value
  Guarded g;
  int rc = 0;
  if (kind == 0) {
    const float* dx = g.in(x, np * ci);
    const float *dw = g.in(w, nw), *dbi = g.in(bias, (size_t)co), *dw2 = g.in(w2, nw), *db2 = g.in(bias2, (size_t)co);
    const float* dres = g.in(aux, np * co);
    float* dout = g.out<float>(np * co, "out");
    if (!g.ok) return -12;
    drq::conv_fwd(pl, dx, dw, dbi, dres, dout, B, (flags & 1) != 0, nullptr, dw2, db2, w2 ? B1 : -1);
    if ((rc = sync_rc("conv_fwd")) || (rc = g.check())) return rc;
    if (!g.back(out, dout, np * co)) return -5;
  } else if (kind == 1) {
    const float *ddout = g.in(x, np * co), *dw = g.in(w, nw), *dmask = g.in(aux, np * ci), *ddres = g.in(aux2, np * ci);
    float* ddin = g.out<float>(np * ci, "din");
    if (!g.ok) return -12;
    drq::conv_bwd_data(pl, ddout, dw, dmask, ddres, ddin, B, nullptr);
    if ((rc = sync_rc("conv_bwd_data")) || (rc = g.check())) return rc;
    if (!g.back(out, ddin, np * ci)) return -5;
  } else {
    const int G = pl.rows, n = (int)nw + co;
    const bool defer = (flags & 2) != 0;
    const float *dx = g.in(x, np * ci), *ddout = g.in(aux, np * co);
    float* part = g.out<float>((size_t)G * n, "part");
    float* ddw = g.out<float>(nw, "dw");
    float* ddb = g.out<float>((size_t)co, "db");
    if (!g.ok) return -12;
    const drq::SumSeg seg{part, ddw, ddb, G, n, (int)nw, 0};
    const drq::SumSeg* dseg = g.in(&seg, 1);
    if (!g.ok) return -12;
    drq::conv_wgrad(pl, dx, ddout, part, ddw, ddb, (flags & 1) != 0, nullptr, defer);
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

// 1: the head entry points below run their forward and data-grad kernels with HeadParams::shared set (every row
// reads block 0 of Wh / bh, whatever its task); the per-task weight kernels read no head parameter and stay
static int g_dbg_head_shared = 0;
int mtsac_debug_head_shared(int on) {
  const int old = g_dbg_head_shared;
  g_dbg_head_shared = on ? 1 : 0;
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
    p.head.B = B; p.head.W = W; p.head.hd = hd; p.head.E = 1; p.head.shared = g_dbg_head_shared;
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
    q.B = B; q.W = W; q.hd = 1; q.E = E; q.shared = g_dbg_head_shared;
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

// ---- the symmetric eigenvalue kernels (symeig.hip) ----
// Accepts arbitrary doubles.  The kernels are written for Grams of fp32 activations: |a_ij| <= 2^24 * 2^256 and
// nonzero entries >= 2^-298, so the squares of a column and their sums stay inside fp64's normal range and the
// reflector's norm is formed without scaling.  Outside that domain a norm may overflow or lose its small
// terms; an overflow ends as a non-finite tridiagonal form, that is an all-NaN row and flag bit 1.
int mtsac_debug_sym_eigvals(int Z, int r, const double* A, double* lam, double* d, double* e, int32_t* flags) {
  if (Z < 1 || Z > 64 || r < 1 || r > SYM_EIG_MAX_ORDER || !A || !lam || !flags) return -22;
  if (!outputs_distinct({lam, d, e, flags})) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const size_t n = (size_t)Z * r * r, Zr = (size_t)Z * r, Ze = (size_t)Z * (r - 1);
  Guarded g;
  SymEig s{};
  // in place: a store outside the matrices shows in the bands, a read past the last one in r words of NaN
  s.A = g.out<double>(n + r, "A");
  if (s.A && hipMemcpy(s.A, A, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) g.ok = false;
  s.Z = Z;
  s.r = r;
  s.d = g.out<double>(Zr, "d");
  s.e = g.out<double>(Ze, "e");
  s.v = g.out<double>(2 * Zr, "v");
  s.p = g.out<double>(2 * Zr, "p");
  s.part = g.out<double>((size_t)Z * sym_tridiag_parts(r), "part");
  s.tau = g.out<double>((size_t)2 * Z, "tau");
  s.lam = g.out<double>(Zr, "lam");
  s.flags = g.out<int>((size_t)Z, "flags");
  if (!g.ok) return -12;
  sym_tridiag(s, nullptr);
  tridiag_eigvals(s, nullptr);
  int rc = 0;
  if ((rc = sync_rc("sym_eigvals")) || (rc = g.check())) return rc;
  if (d && !g.back(d, s.d, Zr)) return -5;
  if (e && Ze && !g.back(e, s.e, Ze)) return -5;
  return g.back(lam, s.lam, Zr) && g.back(flags, s.flags, (size_t)Z) ? 0 : -5;
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
  hp.B = B; hp.W = W; hp.hd = hd; hp.E = E; hp.shared = g_dbg_head_shared;
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

int mtsac_debug_head_backward_shared(int B, int T_l, int E, int W, int hd, const int* task, const float* h,
                                     const float* Wh, const float* dout, float* dz, float* db, float* dWh, float* dbh,
                                     int* info) {
  if (!head_kernels_cover(hd, W) || E < 1 || E > 4 || W < 1 || !h || !Wh || !dout || !dz || !db || !dWh || !dbh || !info ||
      !tasks_ok(task, B, T_l) || (long long)E * B * W >= (1LL << 28) || !outputs_distinct({dz, db, dWh, dbh, info}))
    return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  const int chunks = head_backward_chunks(T_l);
  const size_t nh = (size_t)E * B * W, nw = (size_t)E * W * hd, nd = (size_t)E * B * hd;
  Guarded g;
  TaskLists tl = make_lists(g, task, B, T_l);
  HeadParams hp{};
  hp.h = g.in(h, nh); hp.Wh = g.in(Wh, nw); hp.task = tl.d_task;
  hp.B = B; hp.W = W; hp.hd = hd; hp.E = E; hp.shared = 1;
  hp.sWh = (long long)W * hd; hp.sbh = hd; hp.sh = (long long)B * W;
  hp.fault = g.mem.get<unsigned>(1);  // zeroed
  const float* d_dout = g.in(dout, nd);
  float* d_dz = g.out<float>(nh, "dz");
  float* d_dbp = g.out<float>((size_t)E * chunks * W, "dbp");
  float* d_db = g.out<float>((size_t)E * W, "db");
  float* d_ws = g.out<float>((size_t)head_shared_ws_floats(B, W, hd, E), "ws");
  float* d_dWh = g.out<float>(nw, "dWh");
  float* d_dbh = g.out<float>((size_t)E * hd, "dbh");
  if (!g.ok || !hp.fault) return -12;
  std::fill(info, info + 8, 0);
  const bool data = W % 4 == 0;  // the data pass's contract (kernels.h)
  if (data) {
    head_backward_data(hp, d_dout, (long long)B * hd, d_dz, tl.counts, tl.rows, B, T_l, nullptr, PlaneOut{}, d_dbp);
    colsum_finish(d_dbp, W, chunks, E, d_db, W, nullptr);
  }
  info[0] = data ? 1 : 0;
  info[1] = head_backward_weight_shared(hp, d_dout, (long long)B * hd, d_ws, d_dWh, d_dbh, nullptr) ? 1 : 0;
  info[3] = HEAD_SHARED_ROWS;
  info[4] = head_shared_chunks(B);
  int rc = 0;
  if ((rc = sync_rc("head_backward_shared")) || (rc = g.check())) return rc;
  unsigned fault = 0;
  if (!g.back(&fault, hp.fault, 1)) return -5;
  info[2] = (int)fault;
  return g.back(dz, d_dz, nh) && g.back(db, d_db, (size_t)E * W) && g.back(dWh, d_dWh, nw) &&
                 g.back(dbh, d_dbh, (size_t)E * hd)
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

int mtsac_debug_replay_indices_tasks(uint64_t* state, int64_t size, int T, const int32_t* sizes, int n_alloc,
                                     int32_t* idx) {
  if (!state || !idx || !sizes || T < 1 || T > 64 || size < 0 || size >= (1LL << 31) || n_alloc < 1 ||
      n_alloc > (1 << 24) || (state[4] & ~1ull) || state[5] > 0xFFFFFFFFull)
    return -22;
  std::vector<int> offs(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    if (sizes[t] < 0 || sizes[t] > n_alloc) return -22;
    offs[t + 1] = offs[t] + sizes[t];
    if (offs[t + 1] > n_alloc) return -22;
  }
  const int total = offs[T];
  if (total < 1) return -22;
  if (hipSetDevice(0) != hipSuccess) return -5;
  unsigned long long jt[65 * 4];
  pcg_jump_table(jt);
  PcgDev s{state[0], state[1], state[2], state[3], (int)state[4], (unsigned)state[5]};
  const long long sz = size;
  Guarded g;
  const unsigned long long* d_jump = g.in(jt, (size_t)65 * 4);
  const long long* d_size = g.in(&sz, 1);
  const int* d_sizes = g.in(sizes, (size_t)T);
  const int* d_offs = g.in(offs.data(), (size_t)T + 1);
  PcgDev* d_rng = guarded_inout(g, &s, 1, "rng");
  int* d_idx = g.out<int>((size_t)n_alloc, "idx");
  if (!g.ok) return -12;
  replay_indices_tasks(d_rng, d_jump, d_size, d_sizes, d_offs, T, total, d_idx, nullptr);
  int rc = 0;
  if ((rc = sync_rc("replay_indices_tasks")) || (rc = g.check())) return rc;
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
  if ((src != 0 && src != 1 && src != 2) || n < 1 || T_l < 1 || T_l > 64 || D < 1 || A < 1 || A > 64 || T_glob < 1 || T_glob > D ||
      task_begin < 0 || ld_a < D || ld_c < A + D || R < 2 * D + A + 2 || pm < 0 || pm > 2 || (long long)n * T_l > (1 << 20) ||
      !xa || !xa_next || !xc || !xc_next || !xc_pi || !rew || !done || !task || !err || (rmin == nullptr) != (rmax == nullptr))
    return -22;
  const int B = src != 1 ? n * T_l : n;
  std::vector<int> offs(T_l + 1, 0);
  if (src == 2) {  // task-major: dims[17 + t] rows of task t, one index per row; no reward normalisation
    if (rmin) return -22;
    for (int t = 0; t < T_l; ++t) {
      if (dims[17 + t] < 0 || dims[17 + t] > B) return -22;
      offs[t + 1] = offs[t] + dims[17 + t];
    }
    if (offs[T_l] != B) return -22;
  }
  if (src != 1) {
    if (!store || !idx || cap < 1 || (long long)cap * T_l * R >= (1LL << 27)) return -22;
    for (int i = 0; i < (src == 2 ? B : n); ++i)
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
  p.store = src != 1 ? g.in(store, (size_t)cap * T_l * R) : nullptr;
  p.idx = src != 1 ? g.in(idx, (size_t)(src == 2 ? B : n)) : nullptr;
  p.offs = src == 2 ? g.in(offs.data(), (size_t)T_l + 1) : nullptr;
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
  else if (src == 2) replay_gather_tasks(p, nullptr);
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
