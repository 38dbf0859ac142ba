/*
 * mtsac_debug.h -- test-only entry points of libmtsac.so (not part of the drop-in
 * boundary).  They expose single device kernels so the parity tests can check a
 * kernel in isolation against the oracle / a torch fp32 reference.
 */
#ifndef MTSAC_DEBUG_H_
#define MTSAC_DEBUG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One batched fp32 MFMA GEMM with epilogue on device 0 (host pointers in/out):
 *   kind 0 NN: C = A[M][K] . B[K][N]   kind 1 NT: C = A[M][K] . B[N][K]^T
 *   kind 2 TN: C = A[K][M]^T . B[K][N]
 *   epi 0 store (+ db = column sums of B when kind 2 and db != NULL),
 *   epi 1 relu(acc + bias[n]), epi 2 acc * (mask[m][n] > 0).
 * Every operand is dense with the given leading dimension; batch strides are the
 * dense matrix sizes (A shared across the batch when a_shared != 0).
 * precision: low byte = enum mtsac_precision; bits 8-15 = split-K slices for epi 0
 * (0 or 1: no split). */
int mtsac_debug_gemm(int precision, int kind, int epi, int batch, int M, int N, int K, const float* A, int lda, int a_shared,
                     const float* B, int ldb, float* C, int ldc, const float* bias, const float* mask, int ldm,
                     float* db);

/* Time `iters` back-to-back launches of one GEMM on device-resident random operands
 * (allocated once, dense, lda = K or M as the kind requires); writes the mean
 * milliseconds per launch (HIP events on the launch stream). */
int mtsac_debug_gemm_bench(int precision, int kind, int epi, int batch, int M, int N, int K, int iters,
                           double* ms_per_launch);

/* Pre-split-plane GEMM (gemm_x3p.hip): C[M][N] = op(A) . op(B) from host fp32 arrays.
 * a_kmajor: A given as [K][M] (else [M][K]); b_kmajor: B given as [K][N] (else [N][K]).
 * The operands are split into bf16 planes on the device in their stored orientation and
 * multiplied (k-major operands through the transposed LDS read); epi as in mtsac_debug_gemm
 * (bits 8-15: split-K slices for epi 0).  Csum (nullable): the GEMM also writes C's split
 * planes and Csum receives their sum h + m + l. */
int mtsac_debug_gemm_x3p(int epi, int M, int N, int K, const float* A, int a_kmajor, const float* B, int b_kmajor,
                         float* C, const float* bias, const float* mask, float* Csum);
/* The hidden layers' weight grad in precision split2h alone: per member z < E, C[z][M][N] = A[z]^T . B[z] from
 * host fp32 A [E][K][M] and B [E][K][N] (both k-major).  The fp16 planes are built on the device at the
 * exponents of the operands' maxima, as the engine's producers leave them, and multiplied by the k-major x
 * k-major plain-store launch; slices > 1: split-K into that many slices (<= ceil(K / 32)) and its finishing
 * pass.  C starts as NaN between two guard bands; a written band is an error (-5). */
int mtsac_debug_gemm_x3p_kmajor(int E, int M, int N, int K, int slices, const float* A, const float* B, float* C);
/* Time iters launches of the plane GEMM on device-resident random planes (NT form). */
int mtsac_debug_gemm_x3p_bench(int epi, int batch, int M, int N, int K, int iters, double* ms_per_launch);
/* Select the plane GEMM tile geometry (bits 0-7: 0 = 128x128 k32, 1 = 256x128 k32, 2 = 256x128 k16,
 * 3 = 256x256 k16, 255 = by operand form (default)) and
 * ablation bits for experiments (bits 8-15: plane GEMM, bits 16-23: split GEMM; 0 = normal);
 * returns the old geometry.  Plane GEMM bits: 1 no refill DMA, 2 no MFMAs, 8 refill issued up front (wrong
 * results, timing only), 4 no XCD tile order, 16 the k-major weight grads' unpipelined main loop (the same
 * bits as the pipelined one). */
int mtsac_debug_x3p_geo(int geo);

/* Row-major x row-major plane GEMM (gemm_x3f.hip, 16x16x32 MFMA, K padded to 64): per batch entry
 * C[M][N] = epi(A[M][K] . B[N][K]^T); epi 1 bias+ReLU, 2 ReLU mask (bit 8: mask read from the
 * bf16 high plane of `mask`; bit 9: run gemm_x3s.hip, the small-row-count kernel, instead; bit 10:
 * precision bf16, the products on the operands' high planes only; bit 11: split-K by the
 * launcher's choice, with a workspace, as the engine runs task shards);
 * Csum (nullable): sum of the written output planes.  -95 when the kernel does not take the shape. */
int mtsac_debug_gemm_x3f(int epi, int batch, int M, int N, int K, const float* A, const float* B, float* C,
                         const float* bias, const float* mask, float* Csum);
/* The ragged split2h data grad of the actor step (gemm_x3f_ragged, E = 2) beside the dense launch it
 * replaces, on host arrays at any tile count: A [2][B][K], W [2][N][K], mask [2][B][N], active [2][B]
 * bytes.  Dense: A with the inactive rows zeroed; ragged: the active rows compacted in ascending order.
 * flags bit 0: planes out (else fp32), bit 1: W in the fragment layout.  dense_out / rag_out: fp32
 * [2][B][N] or the two fp16 planes as 16-bit words [2][2][B][N] (ragged: rows at their slots, the rest
 * left at 0xFF bytes); rows_out [2][B]: the lists; info [6]: dense / ragged output exponent, dense /
 * ragged max over the record's partial maxima (float bits; the ragged record starts at 1e30), n_0, n_1. */
int mtsac_debug_gemm_x3f_ragged(int flags, int B, int N, int K, const float* A, const float* W, const float* mask,
                                const unsigned char* active, void* dense_out, void* rag_out, int* rows_out, int* info);
/* Time iters launches of the forward-shaped plane GEMM: which 0 = gemm_x3p (B k-major), 1 = gemm_x3f,
 * -1 = gemm_x3s (-2 / -3: its TI = 7 instance without operand loads / without MFMAs, experiments);
 * epi bits 8-9: outputs 0 = fp32 + planes, 1 = planes only, 2 = fp32 only; bit 10: precision bf16;
 * bit 11: split-K by the launcher's choice (gemm_x3p and gemm_x3f), with a workspace. */
int mtsac_debug_gemm_fwd_bench(int which, int epi, int batch, int M, int N, int K, int iters, double* ms_per_launch);
/* Rows per gemm_x3s tile / 16 (TI, 4..8) the cost model picks for an M x N output, batch entries. */
int mtsac_debug_x3s_ti(int M, int N, int batch);
// The DrQ conv switches (tests, experiments, A/B runs).  They are read when an engine is created and
// when a debug conv entry point below is called -- the one place that plans a conv -- so an engine
// that exists keeps the kernels and buffer sizes it was created with whatever is set afterwards.
// Each setter returns the previous value.
// Channel groups per lane of the one-lane-per-pixel kernels (fwd: output channels, bwd: input
// channels; 0 = the plan's choice); returns fwd | bwd << 8.
int mtsac_debug_drq_groups(int fwd, int bwd);
// The pre-round-6 DrQ conv kernels (one lane per pixel, im2col weight grad) instead of the row-tile
// ones: bit 1 forward, 2 data grad, 4 weight grad; bit 8 runs the row-tile kernels at every shape
// (past the measured per-shape choice); bit 16 turns the split2h MFMA convs off, bit 32 runs them at
// every shape they support.  Default: MTSAC_DRQ_LEGACY in the environment, or 0.  < 0 queries.
int mtsac_debug_drq_legacy(int mask);
// The row-tile conv weight grad's grid cap (> 0 sets, 0 restores the per-shape default, < 0 queries).
int mtsac_debug_drq_wgrad_blocks(int cap);
// Mean microseconds per launch of one DrQ conv pass on random operands: kind 0 forward (ReLU in,
// residual), 1 data gradient (mask, residual), 2 weight-gradient partials.  -22 bad arguments.
int mtsac_debug_drq_conv_bench(int kind, int B, int H, int W, int ci, int co, int iters, double* us_per_launch);

/* Single DrQ kernels on device 0, null stream, host pointers in and out; 0 or a negative errno (-22
 * for bad sizes or an unsupported channel pair, before anything is launched).  Every device output
 * lies between two 256-byte bands of a fixed byte and starts as all-ones words (NaN as float): a
 * written band returns -5 with the buffer named in mtsac_last_error, an element the kernel left
 * alone comes back NaN.  Tests only.
 *
 * One 3x3 / stride 1 / SAME conv pass as the engine launches it (NHWC, kernel [3][3][ci][co]):
 *   kind 0 forward: x input, flags bit 0 relu_in, aux residual (nullable), w2 / bias2 (nullable) the
 *     second parameter set of images [B1, B), out [B][H][W][co];
 *   kind 1 data gradient: x dout, aux mask (nullable), aux2 dres (nullable), out din [B][H][W][ci];
 *   kind 2 weight gradient: x input, aux dout, flags bit 0 relu_in, out dw [3][3][ci][co], out2 db [co];
 *     flags bit 1: the partials are left (defer_sum) and reduced by the one-segment form of the
 *     update's partial-sum launch. */
int mtsac_debug_drq_conv(int kind, int flags, int B, int B1, int H, int W, int ci, int co, const float* x,
                         const float* w, const float* bias, const float* w2, const float* bias2, const float* aux,
                         const float* aux2, float* out, float* out2);
/* The plan of a conv of `kind` at this shape under the current switches: out[0] family (0 one lane
 * per pixel / im2col, 1 row tiles, 2 split2h MFMA), out[1] rows per tile, out[2] tiles per image
 * (0 when not tiled), out[3] grid blocks.  The launchers run from such a plan. */
int mtsac_debug_drq_conv_path(int kind, int B, int H, int W, int ci, int co, int* out);
/* Max pool 3x3 / stride 2 / SAME forward then backward: out, arg [B][Ho][Wo][C] (argmax tap 0..8),
 * din [B][H][W][C] from dout [B][Ho][Wo][C]; C a multiple of 4. */
int mtsac_debug_drq_maxpool(int B, int H, int W, int C, const float* in, float* out, unsigned char* arg,
                            const float* dout, float* din);
/* The C51 trio on head outputs hc_* [B][ldh] = [adv (A Z) | val (Z)] before the biases hb_* [(A + 1) Z],
 * ldh >= (A + 1) Z: the target m [B][Z] and a_next [B] from (hc_n online, hc_t target), q [B][A] of
 * hc_n, then the loss at act from hc_s and m: dh [B][ldh] (columns past (A + 1) Z untouched),
 * loss_b [B], logit_b [B]. */
int mtsac_debug_drq_c51(int B, int A, int Z, int ldh, const float* hc_s, const float* hc_n, const float* hc_t,
                        const float* hb_on, const float* hb_tg, const float* rew, const float* done, const int* act,
                        float gamma_n, float vmin, float vmax, float* m, int* a_next, float* q, float* dh,
                        float* loss_b, float* logit_b);

/* Single SAC head kernels (heads.hip) on device 0, null stream, host pointers in and out, through the launch
 * wrappers of kernels.h (so their dispatch by hd, A, W % 4 and rows per wave runs); 0 or a negative errno (-22
 * for bad sizes, before anything is launched).  Outputs are guarded as the DrQ entries' are: an element a
 * kernel left alone comes back NaN (float) or -1 (int), a written band returns -5.  Entries that take task[B]
 * (local ids < T_l <= 64) build the per-task lists with task_rows on the device (row stride B) and return
 * them: counts [T_l], rows [T_l][B] (-1 past counts[t]).  Tests only.
 *
 * The two launcher choices otherwise read once from the environment: rows per wave of the grouped policy
 * heads and the action grad (1 / 2 / 4; anything else restores MTSAC_HEAD_RW / the choice by grid size), and
 * head_backward_both's form (0 the fused kernel, 1 both passes in one launch; anything else restores
 * MTSAC_HEAD_BWD_SPLIT / the choice by grid size).  Each returns the previous override (-1: none). */
int mtsac_debug_head_rw(int rw);
int mtsac_debug_head_bwd_split(int mode);
/* policy_head: form 0 one wave per row (no lists), 1 grouped by task, 2 policy_head_pair on two row sets
 * (h, eps and every output then hold two sets, [2][...]).  h [B][W], Wh [T_l][W][2A], bh [T_l][2A],
 * eps [B][A] (injected noise, required).  flags bit 0: with WhT from head_transpose; bit 1 / bit 2: the
 * action planes as split3 / split2h (at exponent 14), returned in planes [B][ld_a] as their unscaled sum.
 * a_out, a_out2 [B][ld_a] (ld_a >= A: the columns past A stay NaN), logpi [B], cache [B][5A].  A <= 64; a wide
 * head (A > 4) needs W % 4 == 0.  The output buffers of a call (here and in the head backward and action grad
 * below) must be distinct: each is copied back in turn, so two that share an address are refused (-22). */
int mtsac_debug_head_policy(int form, int flags, int B, int T_l, int W, int A, int ld_a, const int* task, const float* h,
                            const float* Wh, const float* bh, const float* eps, float ls_min, float ls_max,
                            float* a_out, float* a_out2, float* logpi, float* cache, float* planes, int* counts,
                            int* rows);
/* The same launch with eps == NULL in PolicyParams: the heads draw their noise from the device stream,
 * normal4(seed, stream + 16 (lane >> 2), counter, noise_div > 0 ? b / noise_div : b)[lane & 3] for action lane
 * `lane` of row b (devrng.h), stream = stream_id for the first row set and stream_id + 1 for the second of form 2;
 * counter is copied to the device word the heads read.  The drawn noise comes back in cache[:, 4A:5A]. */
int mtsac_debug_head_policy_noise(int form, int flags, int B, int T_l, int W, int A, int ld_a, const int* task,
                                  const float* h, const float* Wh, const float* bh, uint64_t seed, uint32_t stream_id,
                                  uint64_t counter, int noise_div, float ls_min, float ls_max, float* a_out,
                                  float* a_out2, float* logpi, float* cache, float* planes, int* counts, int* rows);
/* critic_head: mode 0 target, 1 critic, 2 actor; flags bit 0 fused_target (mode 1: th / tWh / tbh the target
 * critic's head inputs, y_out written), bit 1 clip.  h [E][B][W], Wh [E][T_l][W], bh [E][T_l], log_alpha
 * [T_glob], y [B] (mode 1 without fused_target), tw [B] or null.  Outputs y_out, row_a, row_b, alpha_w [B],
 * dq [E][B] (what the mode does not write stays NaN), dq_amax [2048] the record's partial maxima and
 * *dq_parts how many the launcher reports. */
int mtsac_debug_head_critic(int mode, int flags, int B, int T_l, int E, int W, int T_glob, int task_begin,
                            const int* task, const float* h, const float* Wh, const float* bh, const float* th,
                            const float* tWh, const float* tbh, const float* rew, const float* done,
                            const float* logpi, const float* log_alpha, const float* y, const float* tw, float gamma,
                            float inv_norm, float* y_out, float* dq, float* row_a, float* row_b, float* alpha_w,
                            float* dq_amax, int* dq_parts);
/* active_rows of dq [E][B]: n [E], rows [E][B] (-1 past n[e]), slot [E][B]. */
int mtsac_debug_head_active_rows(int E, int B, const float* dq, int* n, int* rows, int* slot);
/* The head backward.  form 0: head_backward_data (only when W % 4 == 0, its contract) then
 * head_backward_weight; form 1: head_backward_both; form 2: the compacted data pass (hd = 1, W % 4 == 0, planes:
 * slot from active_rows on dq [E][B]; plane row s of member e is its s-th active row).  h [E][B][W],
 * Wh [E][T_l][W][hd], dout [E][B][hd].  flags bit 0 / bit 1: split3 / split2h planes (bound inputs: max |dout|,
 * max |Wh|, w_add 0, kmul hd), returned in planes [E][B][W] as their unscaled sum.  dz [E][B][W], dbp
 * [E][4 T_l][W] and db [E][W] (colsum_finish of dbp), dWh [E][T_l][W][hd], dbh [E][T_l][hd].  info [8]: 0 whether
 * the data pass / head_backward_both ran, 1 the split2h planes' exponent, 2 the self-check's fault word,
 * 3.. n[e] (form 2). */
int mtsac_debug_head_backward(int form, int flags, int B, int T_l, int E, int W, int hd, const int* task, const float* h,
                              const float* Wh, const float* dout, const float* dq, float* dz, float* dbp, float* db,
                              float* planes, float* dWh, float* dbh, int* counts, int* rows, int* info);
/* A head shared by all tasks (MTSAC_NET_SHARED_HEAD; HeadParams::shared).
 * mtsac_debug_head_shared(on): while on, mtsac_debug_head_policy[_noise], _head_critic and _head_backward run
 * their forward and data-grad kernels with the shared flag -- every row reads block 0 of the Wh / bh passed in,
 * whatever its task (the per-task weight kernels read no head parameter and are unchanged; head_backward_both
 * refuses a shared head).  Returns the previous setting.
 * mtsac_debug_head_backward_shared: Wh [E][W][hd]; the data pass (W % 4 == 0 only; dz [E][B][W] and db [E][W],
 * rows walked by the per-task lists as in a step) and head_backward_weight_shared: dWh [E][W][hd] =
 * sum_b h[e][b][w] dout[e][b][o] and dbh [E][hd] = sum_b dout over ALL B rows.  info [8]: 0 whether the data pass
 * ran, 1 whether the weight pass ran, 2 the self-check's fault word, 3 the weight pass's row chunk R, 4 its
 * chunk count. */
int mtsac_debug_head_shared(int on);
int mtsac_debug_head_backward_shared(int B, int T_l, int E, int W, int hd, const int* task, const float* h,
                                     const float* Wh, const float* dout, float* dz, float* db, float* dWh, float* dbh,
                                     int* info);
/* action_grad: dz1 [E][B][Wc] dense; with dq [E][B] (nullable) the rows are compacted by active_rows' slot
 * first (the dense equivalent has zero rows where dq is 0).  W0 [E][Ic][Wc], cache [B][5A], alpha_w [B];
 * a_data [B][ld_a_data] (nullable) with explore_scale and row_loss_in [B].  Outputs dout [B][2A], row_loss,
 * row_explore [B] (NaN without a_data), dout_amax [2048] and *dout_parts as for the critic head. */
int mtsac_debug_head_action_grad(int B, int E, int Wc, int Ic, int A, const float* dz1, const float* dq, const float* W0,
                                 const float* cache, const float* alpha_w, const float* a_data, int ld_a_data,
                                 float explore_scale, float ls_min, float ls_max, const float* row_loss_in, float* dout,
                                 float* row_loss, float* row_explore, float* dout_amax, int* dout_parts);
/* row_alpha: alpha_row [B] and, with use_tw, tw_row [B] (else left NaN) from log_alpha [T_glob]. */
int mtsac_debug_head_row_alpha(int B, int T_l, int T_glob, int task_begin, int use_tw, const int* task,
                               const float* log_alpha, float* alpha_row, float* tw_row);

/* The trunk GEMMs' bias-grad path and the layout kernels, one launch family at a time: device 0, null stream,
 * host pointers in and out, outputs guarded as the head entries' are (an element left alone comes back NaN, or
 * all-ones words; a written band returns -5 and names the buffer); -22 for bad sizes and -95 for a shape the
 * kernel refuses, both before anything is launched.  Tests only.
 *
 * mtsac_debug_gemm_x3f with the engine's strides: epi bits 0-14 as there, bit 15 planes only (C may be null, the
 * engine's data-grad form).  ld_n >= N (a multiple of 4) is the row stride of the output planes and of the mask
 * planes (bit 8), rows_p >= M the rows allocated per plane (plane stride rows_p * ld_n; A's planes carry zero rows
 * past M); C keeps ldc = N.  K is padded with zero columns to 64 (gemm_x3s, bit 9: to 32, so K = a padded width
 * runs as the engine runs it; the caller's A then holds zeros in the columns past the width).  Csum
 * [batch][rows_p][ld_n]: the sum of the written planes (precision bf16: the high plane), NaN wherever the kernel
 * wrote nothing.  dbp: the column-sum partials as the launch leaves them, [batch][chunks][N] dense at the front of
 * batch * gemm_x3f_max_row_tiles(M) * N floats (= ceil(M / 16) row tiles), the rest NaN; db [batch][N]:
 * colsum_finish of dbp over the chunk count the engine derives for the next weight grad.  info [8]: 0 the family
 * that ran (0 unsplit gemm_x3f, 1 split-K with the in-launch finish, 2 split-K with the finishing pass, 3
 * gemm_x3s), 1 rows per dbp chunk as the engine computes them, 2 chunks = ceil(M / that), 3 K slices, 4 partial
 * maxima the launcher reports, 5 gemm_x3f_max_row_tiles(M), 6 the split2h output exponent, 7 the launch's row
 * tile (gemm_x3s: TI). */
int mtsac_debug_gemm_x3f_ld(int epi, int batch, int M, int N, int K, int ld_n, int rows_p, const float* A,
                            const float* B, float* C, const float* bias, const float* mask, float* Csum, float* dbp,
                            float* db, int* info);
/* The k-major x k-major gemm_x3p weight grad (split3) of E members with the bias grad finished from column-sum
 * partials (SplitGemmParams::cs_part): A [E][K][M], B [E][K][N], part [E][chunks][N], splits (0: the launcher's
 * choice) -> C [E][M][N] = A^T B, db [E][N].  mode 0 finishes at once (colsum_finish, or inside the split-K
 * reduce launch); mode 1 defers the finish to a FinishSink that holds a colsum_job on part_pre [E][nb[0]][nb[1]]
 * before it and one on part_post [E][nb[2]][nb[3]] after it, all run by one finish_many: db_pre [E][nb[1]],
 * db_post [E][nb[3]] come back too (mode 0 ignores nb and the four).  info [4]: 0 K slices used, 1 who finished
 * the bias grad (0 colsum_finish, 1 the reduce launch, 2 finish_many), 2 the sink's jobs, 3 slab-sum blocks of
 * the deferred job. */
int mtsac_debug_wgrad_finish(int mode, int E, int M, int N, int K, int chunks, int splits, const float* A,
                             const float* B, const float* part, const int* nb, const float* part_pre,
                             const float* part_post, float* C, float* db, float* db_pre, float* db_post, int* info);
/* The layout kernels.  kind 0 split_planes: dims [12] = rows, cols, ldx, out_rows, out_cols, ldo, rows allocated
 * per plane (plane stride = that * ldo), transpose, batch, frag, split2h, its exponent; x [batch][rows][ldx];
 * out: the raw 16-bit plane words [batch][3][allocated rows][ldo].  kind 1 transpose_f32: dims = rows, cols,
 * batch; out [batch][cols][rows].  kind 2 colsum: dims = rows, cols, ld, batch; x [batch][rows][ld]; out: part
 * [batch][chunks][cols] dense at the front of batch * 64 * cols floats (chunks = min(64, ceil(rows / 256)), the
 * rest NaN), out2: db [batch][cols]. */
int mtsac_debug_layout(int kind, const int* dims, const float* x, void* out, void* out2);

/* The replay kernels (replay.hip) one launch at a time: device 0, null stream, host pointers in and out, outputs
 * guarded as the head entries' are (an element left alone comes back NaN / -1 / all-ones words, a written band
 * returns -5 and names the buffer); -22 for bad sizes or an index / task id out of range, before anything is
 * launched.  Tests only.
 *
 * The index stream.  state [6] in and out: the PcgDev words state_hi, state_lo, inc_hi, inc_lo, has_uint32,
 * uinteger.  mode 0: replay_indices_high with high = high_or_size; mode 1: replay_indices with *buf_size =
 * high_or_size on the device (high = max(size, n)).  The jump table is pcg_jump_table's, as in the engines.
 * idx [n_alloc], n_alloc >= n: positions >= n must come back -1.  -22 for high >= 2^31. */
int mtsac_debug_replay_indices(uint64_t* state, int mode, int64_t high_or_size, int n, int n_alloc, int32_t* idx);
/* replay_indices_tasks (per-task batch sizes): sizes [T], T <= 64, with *buf_size = size on the device; task t's
 * sizes[t] draws of integers(0, max(size, sizes[t])) land at idx[off[t] ..), off the exclusive prefix sums.  idx
 * [n_alloc], n_alloc >= sum(sizes) >= 1: positions past the sum must come back -1. */
int mtsac_debug_replay_indices_tasks(uint64_t* state, int64_t size, int T, const int32_t* sizes, int n_alloc,
                                     int32_t* idx);
/* replay_gather (dims[0] = 0: store [cap][T_l][R] and idx [n], B = n T_l rows), replay_gather_tasks (dims[0] = 2:
 * the task-major form, idx [B], dims [17 + T_l] with dims[17 + t] = the rows of task t, summing to B = n T_l;
 * rmin / rmax must be NULL) or batch_scatter (dims[0] = 1: the
 * five user arrays of B = n rows, row b of local task b % T_l).  dims [17] = source, n, T_l, cap, obs_dim D,
 * act_dim A, T_glob, task_begin, ld_a, ld_c, plane mode (0 none, 1 split3, 2 split2h with *in_max), pa_ld, pc_ld,
 * pa_next, rows allocated per pa plane, rows allocated per pc / pcn / pcp plane, R.  rmin / rmax [T_l] (both or
 * neither) with norm_eps: the gather's reward normalisation.  Outputs xa, xa_next [B][ld_a], xc, xc_next, xc_pi
 * [B][ld_c], rew, done, task [B], err [1] (starts 0); with planes the raw 16-bit words of pa [np][pa rows][pa_ld]
 * and pc, pcn, pcp [np][pc rows][pc_ld] (np = 3, split2h 2) and *in_rec_e = in_rec->e (split2h). */
int mtsac_debug_replay_gather(const int* dims, const float* store, const int32_t* idx, const float* u_obs,
                              const float* u_act, const float* u_nobs, const float* u_done, const float* u_rew,
                              const double* rmin, const double* rmax, double norm_eps, const float* in_max, float* xa,
                              float* xa_next, float* xc, float* xc_next, float* xc_pi, float* rew, float* done,
                              int32_t* task, int32_t* err, uint16_t* pa, uint16_t* pc, uint16_t* pcn, uint16_t* pcp,
                              int32_t* in_rec_e);
/* task_rows: task [B] (ids < T_l <= 64) -> counts [T_l], rows [T_l][max_rows] (-1 past min(counts[t], max_rows)). */
int mtsac_debug_task_rows(int B, int T_l, int max_rows, const int32_t* task, int32_t* counts, int32_t* rows);
/* buffer_pack_slot then buffer_commit_slot of one slot: obs, nobs [T_l][D], act [T_l][A], rew, done [T_l] -> rec
 * [T_l][R]; rmin / rmax [T_l] in and out (both or neither), *buf_size = size out, *bufmax in and out (nullable). */
int mtsac_debug_pack_commit(int T_l, int D, int A, int R, int64_t size, const float* obs, const float* nobs,
                            const float* act, const float* rew, const float* done, float* rec, double* rmin,
                            double* rmax, int64_t* buf_size, float* bufmax);
/* absmax_into: *m = max(*m, max |x[0..n)|), *m in and out. */
int mtsac_debug_absmax(int64_t n, const float* x, float* m);
/* fill_synthetic: store [cap][T_l][R], R = round_up(2 D + A + 2, 4), and *bufmax in and out. */
int mtsac_debug_fill_synthetic(int64_t cap, int T_l, int D, int A, int T_glob, int task_begin, uint64_t seed,
                               float* store, float* bufmax);

/* Eager update_many overlaps consecutive steps (the next gather and critic(s, a) forward beside
 * the previous actor backward / all-reduce / Adam): on = 1 always, 0 never (whole steps), -1 the
 * default (when the trunk gradients go through a device collective: RCCL or the modelled one).
 * Returns the previous setting.  Tests and experiments. */
struct mtsac_engine;
int mtsac_debug_set_pipeline(struct mtsac_engine* engine, int32_t on);

/* 1 when the engine issues every compute segment on its main stream (the default; the 5-lane
 * form needs MTSAC_LANES=1 and enough hardware queues: GPU_MAX_HW_QUEUES as the process started
 * >= 5 per live engine + 3), else 0. */
int mtsac_debug_lane_mode(struct mtsac_engine* engine);
/* The form optimize() gives one network's clip / Adam / Polyak pass (which 0 actor, 1 critic), through
 * the predicates it uses itself: bits 0-1 the trunk kernels' form (0 elementwise only, 1 flat plane
 * segments, 2 64x64 tiles writing natural and transposed planes); bit 4 the head pass writes the
 * transposed head kernel (AdamParams::whT); bit 5 the network ran the sharded optimizer in the last
 * step issued.  Tests only. */
int mtsac_debug_opt_form(struct mtsac_engine* engine, int which);
/* Guard zones (MTSAC_GUARD_BYTES=n in the environment before the engine is created): n bytes of 0xFF
 * around every device allocation.  Returns the number of guards a kernel wrote (0 = intact; -95 when
 * the mode is off); the first few are named in mtsac_last_error. */
int mtsac_debug_check_guards(struct mtsac_engine* engine);
/* Step buffer views (diagnostics): snapshot on/off; read id 0 actor top activations, 1 / 2 their
 * snapshots after the actor forward / the actor-loss pass ([Ma][W]), 3 actor dout ([B][2A]), 4 actor
 * gradient head leaves, 5 the actor-loss pass's policy cache of the last step ([B][5A]: mu, ls, x, a, eps; the
 * actor backward reads it and nothing writes it again before the next step).  count must equal the buffer's
 * float count. */
int mtsac_debug_snapshot(struct mtsac_engine* engine, int32_t on);
int mtsac_debug_read(struct mtsac_engine* engine, int32_t id, float* dst, int64_t count);
/* the head backward's LDS self-check, tested: the last step's actor head weight pass re-run into a
   scratch output with one cross-wave LDS slot corrupted on purpose; the next mtsac_get_logs /
   mtsac_synchronize must fail (-5, "head backward self-check failed").  Needs a step first. */
int mtsac_debug_head_selfcheck(struct mtsac_engine* engine);
/* Weight planes in the fragment layout (gemm_x3f B operand, engine.cpp Net::bfrag): mode -1 (the
 * default) decides by shape (MTSAC_BFRAG=0 turns it off), 0 / 1 forces it off / allows it, for
 * engines created afterwards.  mtsac_debug_bfrag: bit i actor layer i, bit 8 + i critic layer i. */
int mtsac_debug_set_bfrag(int32_t mode);
/* The actor step's pass through the critic over each member's active rows only (rows whose dq is not
 * zero; engine.cpp actor_compact): mode -1 (the default) follows MTSAC_ACTOR_DENSE (1: the dense pass),
 * 0 / 1 forces compacted-where-it-applies / dense, for engines created afterwards. */
int mtsac_debug_set_actor_dense(int32_t mode);
/* 1 when the last step this engine issued (or captured) ran that pass compacted, else 0. */
int mtsac_debug_actor_compact(struct mtsac_engine* engine);
int mtsac_debug_bfrag(struct mtsac_engine* engine);
/* on != 0: this engine issues on one stream whatever MTSAC_LANES asks, and is not counted by the
 * lane grant of the other live engines (experiments comparing the two issue forms in one process). */
int mtsac_debug_force_one_stream(struct mtsac_engine* engine, int32_t on);
/* Modelled trunk-gradient collective for one-GPU runs of a task shard: with nranks > 1 the engine
 * takes its sharded path and, at every point where it would call RCCL, issues on the collective
 * stream a delay of 2 (nranks - 1) / nranks * bucket bytes / bus_gbps (GB/s) held by
 * (flags >> 8) & 255 workgroups (0: 8); the data stay as they are (a one-rank sum).  flags bit 0:
 * the bucket reads NaN until the delay is over (a consumer without a stream edge to the
 * collective turns the step into NaN).  nranks = 1 switches it off.  Not with a communicator or hook. */
int mtsac_debug_set_collective_model(struct mtsac_engine* engine, int32_t nranks, double bus_gbps, int32_t flags);

/* Per-launch record of the last timed step (mtsac_set_timing): i < 0 returns the number of
 * records; else dims = {family = GEMM kind, M, N, K, batch} and *ms its duration. */
struct mtsac_engine;
int mtsac_debug_timed_launch(struct mtsac_engine* engine, int32_t i, int32_t* dims, double* ms);

/* The two network-metrics kernels alone (netmetrics.hip) on host arrays: Z matrices of M rows x W columns, H
 * [Z][M][ld] (ld >= W; the padding columns are never read, and the device copy is followed by M more rows of
 * NaN).  Outputs start as NaN / -1 between guard bands; -5 on a written band (named in mtsac_last_error).
 * mtsac_debug_act_stats: score [Z][W] = mean_b |H|, norm [Z][W] = score / (mean_j score + 1e-9), count [Z] =
 * #(norm <= threshold).
 * mtsac_debug_act_gram: gram [Z][r][r] fp64, r = min(M, W); info[0] = the side formed (0: H^T H, 1: H H^T),
 * info[1] = r. */
int mtsac_debug_act_stats(int Z, int M, int W, int ld, const float* H, float threshold, float* score, float* norm,
                          int32_t* count);
int mtsac_debug_act_gram(int Z, int M, int W, int ld, const float* H, double* gram, int32_t* info);
/* HIP-event durations of the last mtsac_network_metrics call's kernels: ms[0] the column statistics of every
 * layer, ms[1] the Grams (0 for a part the call did not run). */
int mtsac_debug_network_metrics_ms(struct mtsac_engine* engine, double* ms /* 2 */);

/* The two symmetric-eigenvalue kernels alone (symeig.hip) on host arrays: Z symmetric
 * matrices A [Z][r][r] (both triangles, read only from the caller's side; the device copy is reduced in place
 * between guard bands and followed by r words of NaN).  lam [Z][r] ascending, flags [Z] (bit 0: a non-finite
 * entry, bit 1: a non-finite tridiagonal form; either gives an all-NaN row); d [Z][r], e [Z][r-1] the
 * tridiagonal form, each may be NULL.  -22 for Z < 1, Z > 64, r < 1, r > 8192 or a NULL A, lam or flags.
 * Accepts arbitrary doubles; the kernels are written for Grams of fp32 activations, |a_ij| <= 2^24 * 2^256 with
 * nonzero entries >= 2^-298, where the squares of a column and their sums stay inside fp64's normal range. */
int mtsac_debug_sym_eigvals(int Z, int r, const double* A, double* lam, double* d, double* e, int32_t* flags);
/* HIP-event durations of the last mtsac_network_eigvals call for `which`: ms[0] the reduction to tridiagonal
 * form, ms[1] the bisection; launches: the kernel launches and memsets of that call (may be NULL). */
int mtsac_debug_network_eigvals_ms(struct mtsac_engine* engine, int which, double* ms /* 2 */, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif
