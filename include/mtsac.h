/*
 * mtsac.h -- C-ABI of the MI355X multi-task SAC update engine (libmtsac.so).
 *
 * Drop-in boundary for the reference's MTSAC hot path.  Every entry point
 * cites the reference interface it replaces (paths relative to the
 * reginald-mclean/mtrl tree):
 *
 *   mtsac_create / mtsac_destroy   MTSAC.initialize      mtrl/rl/algorithms/mtsac.py:153-284
 *                                  (device state instead of a flax PyTree)
 *   mtsac_set_params/get_params    TrainState params / opt_state leaves
 *                                  mtrl/rl/algorithms/utils.py:11-46, mtsac.py:197-256
 *   mtsac_buffer_add[_stream]      MultiTaskReplayBuffer.add        mtrl/rl/buffers.py:426-474
 *   mtsac_buffer_write             MultiTaskReplayBuffer.load_checkpoint data  buffers.py:326-335
 *   mtsac_buffer_read              MultiTaskReplayBuffer.checkpoint data       buffers.py:308-324
 *   mtsac_buffer_set/get_state     pos / full fields                buffers.py:306,337-343
 *   mtsac_rng_set / mtsac_rng_get  buffer _rng PCG64 state          buffers.py:260,323,335
 *   mtsac_sample                   MultiTaskReplayBuffer.sample(int) buffers.py:494-549
 *   mtsac_update                   MTSAC.update -> _update_inner     mtsac.py:1173-1251
 *   mtsac_get_logs                 the update's LogDict              mtsac.py:1241-1247
 *   mtsac_eval_action              MTSAC.eval_action / _eval_action  mtsac.py:80-84,306-311
 *   mtsac_sample_action            MTSAC.sample_action               mtsac.py:70-77,298-304
 *   mtsac_comm_*                   (new) task-sharded data parallelism over RCCL; the
 *                                  reference is single-device
 *
 * Conventions
 *   - Return value: 0 on success, a negative errno-style code on failure; the
 *     thread-local message is available from mtsac_last_error().  Nothing aborts.
 *   - The engine owns all device memory.  Callers own every pointer they pass;
 *     pointers are borrowed for the duration of the call only.  Data pointers may
 *     be host or device (HIP unified addressing: hipMemcpyDefault).
 *   - One engine per GPU per process.  All work of an engine is serialised on its
 *     own HIP stream; mtsac_get_logs / mtsac_sample / mtsac_get_params are the
 *     synchronisation points.
 *   - Parameter vectors use the flax leaf order (ravel_pytree order) of the
 *     reference networks: head bias, head kernel, layer_0 bias, layer_0 kernel,
 *     layer_1 ... (critic leaves carry the leading ensemble axis).  With task
 *     sharding (task_count < num_tasks) the head leaves hold only the local tasks.
 */
#ifndef MTSAC_H_
#define MTSAC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTSAC_ABI_VERSION 1
#define MTSAC_NUM_LOGS 10

/* log slots, order of mtsac.py:1241-1247 (critic, actor, alpha logs) */
enum mtsac_log_slot {
  MTSAC_LOG_QF_VALUES = 0,          /* losses/qf_values                */
  MTSAC_LOG_QF_LOSS = 1,            /* losses/qf_loss                  */
  MTSAC_LOG_CRITIC_GRAD_NORM = 2,   /* metrics/critic_grad_magnitude   */
  MTSAC_LOG_CRITIC_PARAMS_NORM = 3, /* metrics/critic_params_norm      */
  MTSAC_LOG_ACTOR_LOSS = 4,         /* losses/actor_loss               */
  MTSAC_LOG_ACTOR_GRAD_NORM = 5,    /* metrics/actor_grad_magnitude    */
  MTSAC_LOG_ACTOR_PARAMS_NORM = 6,  /* metrics/actor_params_norm       */
  MTSAC_LOG_EXPLORE_LOSS = 7,       /* metrics/explore_loss (always 0) */
  MTSAC_LOG_ALPHA_LOSS = 8,         /* losses/alpha_loss               */
  MTSAC_LOG_ALPHA = 9               /* alpha = sum(exp(log_alpha))     */
};

/* which parameter / optimizer vector mtsac_{get,set}_params addresses */
enum mtsac_tensor {
  MTSAC_ACTOR = 0,
  MTSAC_CRITIC = 1,
  MTSAC_CRITIC_TARGET = 2,
  MTSAC_LOG_ALPHA_PARAMS = 3,
  MTSAC_ACTOR_ADAM_MU = 4,
  MTSAC_ACTOR_ADAM_NU = 5,
  MTSAC_CRITIC_ADAM_MU = 6,
  MTSAC_CRITIC_ADAM_NU = 7,
  MTSAC_ALPHA_ADAM_MU = 8,
  MTSAC_ALPHA_ADAM_NU = 9
};

enum mtsac_precision {
  MTSAC_FP32 = 0,       /* f32-input MFMA (v_mfma_f32_32x32x2_f32), fp32 everywhere          */
  MTSAC_FP32_SPLIT3 = 1, /* fp32-accurate trunk GEMMs on bf16 MFMA: each fp32 operand split
                           exactly into 3 bf16 terms, 6 cross products accumulated in fp32
                           (dropped terms <= 2^-23 relative); everything else fp32           */
  MTSAC_BF16 = 2,        /* perf-only: the trunk GEMMs' operands rounded to bf16 (the high
                           term of the same split), one bf16 MFMA per product, fp32
                           accumulation; master weights, Adam, heads, losses stay fp32.
                           NOT the reference's arithmetic (fp32): losses drift ~1e-3 rel  */
  MTSAC_FP32_SPLIT2H = 3 /* fp32-accurate trunk GEMMs on fp16 MFMA: each operand tensor scaled
                           by a power of two 2^e (per tensor, from an a-priori bound of its
                           values) and split into 2 fp16 terms (22 significant bits),
                           3 cross products (h*l, l*h, h*h) accumulated in fp32, unscaled
                           exactly; same GEMM error bound as split3 (<= 4e-6 sum|a b|)      */
};

/* Hyper-parameters: MTSACConfig (mtsac.py:116-127) + AlgorithmConfig
 * (config/rl.py:16-22) + ContinuousActionPolicyConfig / QValueFunctionConfig
 * (config/networks.py:6-31) + MultiHeadConfig (config/nn.py:8-31,63) +
 * OptimizerConfig (config/optim.py:14-43) + OffPolicyTrainingConfig
 * (config/rl.py:47-50). */
typedef struct mtsac_config {
  int32_t num_tasks;        /* T: width of the one-hot at the end of obs       */
  int32_t task_begin;       /* first task owned by this engine (sharding)      */
  int32_t task_count;       /* tasks owned by this engine (= T unsharded)      */
  int32_t obs_dim;          /* observation width incl. one-hot (39 + T)        */
  int32_t action_dim;       /* A (4); 1 .. 64 (A > 4: the wide head kernels)    */
  int32_t actor_width, actor_depth;
  int32_t critic_width, critic_depth;
  int32_t num_critics;      /* ensemble size (2)                               */
  int32_t batch_per_task;   /* B / T (128)                                     */
  int64_t capacity;         /* slots per task = buffer_size // T               */
  float gamma, tau;
  float actor_lr, critic_lr, alpha_lr;
  float actor_max_grad_norm, critic_max_grad_norm, alpha_max_grad_norm; /* < 0 (None): no
                               clip; >= 0: optax clip_by_global_norm, 0 included (config/optim.py:38) */
  float adam_b1, adam_b2, adam_eps;
  float initial_temperature;
  float log_std_min, log_std_max;
  int32_t clip;             /* clip y and Q to +-5000 (mtsac.py:557-560)        */
  int32_t use_task_weights; /* mtsac.py:103-113                                 */
  int32_t normalize_rewards;/* 0 off, 1 per-task min/max (buffers.py:534-538), 2 return
                               normalisation (buffers.py:392-422, 531-533): rewards divided
                               by the per-task denominator the host sets through
                               mtsac_buffer_set_reward_stats(min = 0, max = denominator) */
  int32_t precision;        /* enum mtsac_precision                             */
  uint64_t noise_seed;      /* device N(0,1) stream used when no eps is injected */
} mtsac_config;

/* A batch laid out like ReplayBufferSamples (types.py:49-54): rows of this
 * engine's tasks, row = i * task_count + local_task. */
typedef struct mtsac_batch {
  const float* observations;      /* [B_local][obs_dim]    */
  const float* actions;           /* [B_local][action_dim] */
  const float* next_observations; /* [B_local][obs_dim]    */
  const float* dones;             /* [B_local]             */
  const float* rewards;           /* [B_local]             */
} mtsac_batch;

typedef struct mtsac_engine mtsac_engine;

const char* mtsac_last_error(void);
int mtsac_abi_version(void);
/* Build provenance: the first 16 hex digits of the sha256 of the sources the library was built from
 * (the .hip, .cpp and .h files of mtrl_amd/csrc and the .h files of include, in sorted relative-path
 * order, concatenated; mtrl_amd/csrc/Makefile). */
const char* mtsac_build_stamp(void);
void mtsac_default_config(mtsac_config* cfg, int32_t num_tasks);

int mtsac_create(const mtsac_config* cfg, int hip_device, mtsac_engine** out);
/* mtsac_create with network flags (mtsac_create is flags = 0).
 * MTSAC_NET_SHARED_HEAD: actor and critic are the reference's VanillaNetwork -> MLP (mtrl/nn/base.py:11-89):
 * depth Dense+ReLU layers layer_0 .. layer_{D-1} and ONE Dense head layer_D shared by all tasks (the one-hot
 * task columns are inputs only).  Parameter, moment and target vectors then use the flax leaf order of that
 * tree: layer_0/bias, layer_0/kernel, ..., layer_D/bias, layer_D/kernel (critic leaves with the leading ensemble
 * axis): the head [E](hd,) / [E](W, hd) comes LAST, and the per-task gradient matrices have the same columns.
 * Every step form, the rollout calls, the per-task gradient pass and the three gradient-surgery modes run on
 * it; the log slots are unchanged.  -95 with task sharding (task_count < num_tasks); the collective entry
 * points (mtsac_comm_init with nranks > 1, the hooks) return -95 on such an engine.  DESIGN.md section 17.
 * mtsac_shared_head: 1 when the engine was created with the flag. */
#define MTSAC_NET_SHARED_HEAD 1u
int mtsac_create_flags(const mtsac_config* cfg, uint32_t flags, int hip_device, mtsac_engine** out);
int mtsac_shared_head(const mtsac_engine* h);
void mtsac_destroy(mtsac_engine* h);

/* parameters / optimizer state, flax leaf order, fp32 */
int64_t mtsac_param_count(const mtsac_engine* h, int which);
int mtsac_set_params(mtsac_engine* h, int which, const float* src, int64_t n);
int mtsac_get_params(mtsac_engine* h, int which, float* dst, int64_t n);
int mtsac_set_adam_count(mtsac_engine* h, int which /*0 actor,1 critic,2 alpha*/, int32_t count);
int mtsac_get_adam_count(mtsac_engine* h, int which, int32_t* count);

/* replay buffer (device resident; layout documented in DESIGN.md).
 * buffer_add (buffers.py:426-474) does not block the host: the T_local rows are staged through
 * a pinned ring and written + committed on the engine stream, ordered after every update issued
 * before it and before every update issued after it.  Pass the five arrays all in host memory
 * or all in device memory.  Device arrays are read after the work already queued on the
 * producer stream (mtsac_buffer_add: the legacy default stream; mtsac_buffer_add_stream: the
 * hipStream_t passed as producer_stream, e.g. torch.cuda.current_stream().cuda_stream), and
 * the producer stream is made to wait for that read, so the caller may free or overwrite the
 * arrays right after the call.  Reward min / max (normalize_rewards) are kept on the device. */
int mtsac_buffer_add(mtsac_engine* h, const float* obs, const float* next_obs, const float* actions,
                     const float* rewards, const float* dones);
int mtsac_buffer_add_stream(mtsac_engine* h, const float* obs, const float* next_obs, const float* actions,
                            const float* rewards, const float* dones, void* producer_stream);
int mtsac_buffer_write(mtsac_engine* h, int64_t slot_begin, int64_t n_slots, const float* obs,
                       const float* next_obs, const float* actions, const float* rewards,
                       const float* dones);
int mtsac_buffer_read(mtsac_engine* h, int64_t slot_begin, int64_t n_slots, float* obs, float* next_obs,
                      float* actions, float* rewards, float* dones);
int mtsac_buffer_fill_synthetic(mtsac_engine* h, uint64_t seed);
int mtsac_buffer_set_state(mtsac_engine* h, int64_t pos, int32_t full);
int mtsac_buffer_get_state(mtsac_engine* h, int64_t* pos, int32_t* full);
/* normalize_rewards 1: the running per-task reward min / max; 2: (0, denominator) */
int mtsac_buffer_set_reward_stats(mtsac_engine* h, const double* min_r, const double* max_r);
int mtsac_buffer_get_reward_stats(mtsac_engine* h, double* min_r, double* max_r);
int mtsac_rng_set(mtsac_engine* h, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                  uint64_t inc_lo, int32_t has_uint32, uint32_t uinteger);
int mtsac_rng_get(mtsac_engine* h, uint64_t* state_hi, uint64_t* state_lo, uint64_t* inc_hi,
                  uint64_t* inc_lo, int32_t* has_uint32, uint32_t* uinteger);
/* draw one batch with the device index stream and copy it (and the indices) out */
int mtsac_sample(mtsac_engine* h, int64_t* indices, float* obs, float* actions, float* next_obs,
                 float* dones, float* rewards);

/* ---- per-task batch sizes (MultiTaskReplayBuffer.sample with an array, mtrl/rl/buffers.py:494-519; the
 * sizes the reference's Sampler / AdaptiveSampler produce, mtrl/rl/sampling_algs.py).  DESIGN.md section 18.
 * mtsac_set_task_batch_sizes: sizes [T] with sizes[t] >= 0, sizes[t] <= capacity and sum == batch_per_task * T
 * (else -22); NULL: back to the balanced sampler.  While set, the step's OWN device sampling -- mtsac_sample,
 * mtsac_update(batch = NULL), mtsac_update_many -- draws, for t = 0 .. T-1 with sizes[t] > 0, what
 * rng.integers(0, max(buffer_size, sizes[t]), size=sizes[t]) draws, on the one PCG64 stream (the buffered 32-bit
 * half and every rejection carry over from task to task; a task of size 0 makes no call), and returns the rows
 * task by task: row off[t] + j = store[idx_t[j]][t], off the exclusive prefix sums.  mtsac_sample's `indices`
 * then has one entry per row ([batch_per_task * T], task-major).  Rewards are RAW on this path whatever
 * normalize_rewards says: only the reference's int branch normalises.  mtsac_task_gradients and
 * mtsac_network_metrics with batch == NULL keep sampling balanced, interleaved rows.
 * -95 on a task-sharded engine (and from the step calls when collectives are attached afterwards) and while
 * PCGrad, CAGrad or GradNorm is on; their setters return -95 while sizes are set.  The sizes live in device
 * memory (counts, exclusive offsets, contiguous row lists) at fixed addresses: setting or clearing the mode drops
 * a captured step graph, new sizes alone do not, and mtsac_enable_graph(1) works in this mode -- the replayed
 * steps are bit-identical to eager ones.  The device noise of the plain step is drawn per row (it never shared
 * draws across the tasks of a sample index), so row b of an uneven batch reads the stream balanced row b reads.
 * mtsac_get_task_batch_sizes: the sizes in force (batch_per_task each when none are set); returns 1 when set,
 * 0 when balanced.
 * mtsac_set_task_loss_logging: on = 1 adds one launch to the plain step that reduces its per-row loss terms per
 * task in a fixed order (no atomics); default off, the step then launches nothing new.  Switching drops a
 * captured step graph.  mtsac_get_task_losses: out[0][t] = the mean over task t's rows and the ensemble of
 * w (Q_e - y)^2, out[1][t] = the mean over its rows of w (alpha logpi - min_e Q_e), of the last plain step
 * (any batch source); 0 for a task without rows; -22 when logging was never on. */
int mtsac_set_task_batch_sizes(mtsac_engine* h, const int32_t* sizes /* [T] or NULL */);
int mtsac_get_task_batch_sizes(mtsac_engine* h, int32_t* sizes /* [T] */);
int mtsac_set_task_loss_logging(mtsac_engine* h, int32_t on);
int mtsac_get_task_losses(mtsac_engine* h, float* out /* [2][T] */);

/* one gradient step.  batch == NULL: sample from the device buffer.
 * eps_next / eps_cur ([B_local][A] N(0,1) noise for a' ~ pi(.|s') and a ~ pi(.|s));
 * both NULL: device counter-based normal stream. */
int mtsac_update(mtsac_engine* h, const mtsac_batch* batch, const float* eps_next, const float* eps_cur);
/* run `steps` device-sampled, device-noise updates (hipGraph replay when enabled) */
int mtsac_update_many(mtsac_engine* h, int32_t steps);
int mtsac_get_logs(mtsac_engine* h, float* logs /* MTSAC_NUM_LOGS */);
int mtsac_enable_graph(mtsac_engine* h, int32_t enable);
int mtsac_synchronize(mtsac_engine* h);

/* rollout side */
int mtsac_eval_action(mtsac_engine* h, const float* obs, int32_t n, float* actions);
int mtsac_sample_action(mtsac_engine* h, const float* obs, int32_t n, const float* eps, float* actions);

/* multi-GPU: RCCL communicator over the shared-trunk gradients */
int mtsac_comm_unique_id_size(void);
int mtsac_comm_get_unique_id(void* id_out);
/* mtsac_comm_init waits for every peer (MTSAC_COMM_INIT_TIMEOUT_S in the environment bounds the
 * wait); mtsac_comm_init_timeout returns -110 (ETIMEDOUT) when the peers have not joined within
 * timeout_s seconds (<= 0: wait forever) and leaves the engine without a communicator. */
int mtsac_comm_init(mtsac_engine* h, const void* unique_id, int32_t nranks, int32_t rank);
int mtsac_comm_init_timeout(mtsac_engine* h, const void* unique_id, int32_t nranks, int32_t rank,
                            double timeout_s);
/* device noise stream (used when no eps is injected): seed and step counter; setting them
 * rebuilds the step graph (checkpoint / resume of the update noise) */
int mtsac_get_noise_state(mtsac_engine* h, uint64_t* seed, uint64_t* counter);
int mtsac_set_noise_state(mtsac_engine* h, uint64_t seed, uint64_t counter);
/* ranks in the engine's communicator as RCCL reports them (ncclCommCount); 1 without one */
int mtsac_comm_nranks(mtsac_engine* h, int32_t* nranks);
/* Bring-your-own collective: when no RCCL communicator is set, the engine calls
 * fn(user, device_buffer, count) at each all-reduce point (after synchronising its
 * stream), at the same points and in the same order as the RCCL path: one bucket per hidden
 * layer as its weight gradient completes, then layer 0 and the scalar tail; fn must leave the
 * element-wise SUM over all shards in the buffer (completed on the device) before returning.
 * Disables hipGraph replay for this engine.  fn == NULL removes it. */
typedef int (*mtsac_allreduce_fn)(void* user, float* device_buffer, int64_t count);
int mtsac_set_allreduce_hook(mtsac_engine* h, mtsac_allreduce_fn fn, void* user);
/* The same with the sharded optimizer's collectives too: fn(user, op, device_buffer, count), op 0 =
 * all-reduce (sum), 1 = reduce-scatter in place (rank r's shard [r count / world, (r + 1) count / world)
 * of the buffer must hold the element-wise sum over all ranks; the rest is left undefined), 2 =
 * all-gather in place (every rank's shard of the buffer from its owner).  rank / world: this engine's
 * place in the group.  Replaces an all-reduce hook; fn == NULL removes it. */
typedef int (*mtsac_collective_fn)(void* user, int32_t op, float* device_buffer, int64_t count);
int mtsac_set_collective_hook(mtsac_engine* h, mtsac_collective_fn fn, void* user, int32_t rank, int32_t world);
/* Sharded trunk optimizer (ZeRO-1 style) for task-sharded runs (reference OptimizerConfig.spawn /
 * TrainState.apply_gradients, mtrl/config/optim.py:26-43, mtrl/rl/algorithms/utils.py:11-46): every trunk
 * bucket is reduce-scattered instead of all-reduced, the global clip norm comes from an all-reduced
 * |g|^2, each rank runs Adam on its 1/world of the trunk, the new trunk is all-gathered and every
 * rank writes its own GEMM planes and Polyak target from it.  on: 1 / 0; active only with an RCCL
 * communicator or a collective hook (not the one-GPU modelled collective, whose collectives move no data),
 * with world > 1, at most 7 trunk buckets and world dividing every bucket into whole float4s (else the
 * all-reduce path runs).  Switching drops a captured step graph.  The Adam moments then live sharded:
 * get_params of a moment returns this rank's shards current, the rest stale.  Default off (MTSAC_ZERO=1
 * turns it on). */
int mtsac_set_sharded_optimizer(mtsac_engine* h, int32_t on);
/* plain device/host copy helper for hooks written in a host language (hipMemcpyDefault) */
int mtsac_memcpy(void* dst, const void* src, int64_t bytes);

/* measurement: per-kernel-family HIP event timing (events on each launch's own stream) over all
 * steps of the last update / update_many call.  enable: 0 off, 1 on (the step keeps its
 * concurrent streams; forces eager issue), 2 on with every kernel serialised on one stream (solo
 * kernel durations).  Families (enum mtsac_gemm_family):
 * hidden-layer forward, hidden-layer data grad, hidden-layer weight grad, input-layer forward,
 * input-layer weight grad. */
enum mtsac_gemm_family {
  MTSAC_FAM_FORWARD = 0,
  MTSAC_FAM_DATA_GRAD = 1,
  MTSAC_FAM_WEIGHT_GRAD = 2,
  MTSAC_FAM_INPUT_FORWARD = 3,
  MTSAC_FAM_INPUT_WEIGHT_GRAD = 4
};
int mtsac_set_timing(mtsac_engine* h, int32_t enable);
int mtsac_get_timing(mtsac_engine* h, int32_t family, double* total_ms, int32_t* launches,
                     double* flops);
/* the kernel behind a GEMM family at its last launch (labels for the bench and profiles) */
int mtsac_get_timing_kernel(mtsac_engine* h, int32_t family, char* buf, int32_t n);

/* ---- eval-time gradient-conflict statistics (MTSAC.compute_weights, mtsac.py:870-1170;
 * compute_gram_metrics :733-771, compute_support_metrics :774-867; vmap_cos_sim /
 * compute_conflict_metrics, algorithms/utils.py:49-174).  Unsharded engines only (-95).
 * mtsac_task_gradients: per-task gradients of each task's own loss (critic MSE over its n rows,
 * actor loss over its rows) on the CURRENT parameters, into device matrices [T][P] in flax ravel
 * order (which 0 = critic, P = mtsac_task_gradient_size(h, 0); 1 = actor).  batch NULL = sample
 * on device; rows must be interleaved i*T + t (as MultiTaskReplayBuffer.sample returns them).
 * eps_next (the reference samples these from pi(.|s), mtsac.py:1000-1004) / eps_cur: [B][A]
 * injected noise, or both NULL (device noise).  Nothing is updated.
 * mtsac_task_gradient_select: values[t*2+k] = the ranks[t*2+k]-th smallest |g_t| (0-based),
 * the two order statistics of jnp.quantile's linear interpolation.
 * mtsac_task_gradient_stats: one pass over G with support S_t = |g_t| >= thresholds[t]:
 * gram[T*T] = G G^T, l1[T] = sum |g_t|, counts[4][T*T] = #(g_i g_j < 0), #(S_i & S_j),
 * #(S_i & S_j & g_i g_j < 0), #(|g_i| < eps & |g_j| > tau); near_zero[T] = #(|g_t| < eps).
 * The T x T algebra on top is host code (mtrl_amd/conflict.py). */
int mtsac_task_gradients(mtsac_engine* h, const mtsac_batch* batch, const float* eps_next,
                         const float* eps_cur);
int64_t mtsac_task_gradient_size(const mtsac_engine* h, int which);
int mtsac_get_task_gradients(mtsac_engine* h, int which, float* dst, int64_t n);
int mtsac_set_task_gradients(mtsac_engine* h, int which, const float* src, int64_t n);
int mtsac_task_gradient_select(mtsac_engine* h, int which, const int64_t* ranks, float* values);
int mtsac_task_gradient_stats(mtsac_engine* h, int which, const float* thresholds, float eps,
                              float tau, double* gram, double* l1, int64_t* counts,
                              int64_t* near_zero);

/* ---- PCGrad gradient surgery (PCGradConfig on both optimizers, mtrl/config/optim.py and
 * mtrl/optim/pcgrad.py:38-134; the split losses of mtsac.py:513-711).  DESIGN.md section 9.
 * mtsac_set_pcgrad: on = 1 makes mtsac_update / mtsac_update_many run the PCGrad step for BOTH networks
 * (the only combination the reference runs): per-task gradients of critic and actor (mtsac_task_gradients'
 * pass), surgery in Gram form, then the usual clip + Adam (+ Polyak).  Allocates the [T][P] matrices.
 * -95 on a sharded engine or with use_task_weights, -22 for more than 64 tasks, -12 when the matrices do
 * not fit.  The step is eager: mtsac_enable_graph(1) returns -95 while the mode is on.  Log slots 2 and 5
 * hold the pre-surgery |mean_t g_t|, slot 7 the mean explore loss of the split actor loss.
 * mtsac_pcgrad_set_order: pins the task orders (permutations of 0..T-1; jax.random.permutation of the
 * reference) of the following steps; both NULL: back to per-step draws from the device noise stream.
 * mtsac_pcgrad_get_order: the orders the last step used.
 * mtsac_get_pcgrad_logs: out[0..4] the critic's PCGradState of the last step (n_grad_conflicts,
 * avg_grad_magnitude, avg_grad_magnitude_before_surgery, avg_cosine_similarity,
 * avg_cosine_similarity_diff; the last two NaN without cosine_sim_logs), out[5..9] the actor's.
 * The kernels alone, on the matrix mtsac_set_task_gradients / mtsac_task_gradients left (which 0 = critic,
 * 1 = actor): mtsac_task_gram: gram[T*T] = M M^T in fp64; mtsac_task_pcgrad_solve: Gram + solve with the
 * order perm: w[T] (the combine weights, original task order) and logs[6] (the five values above, then
 * |mean_t g_t|); mtsac_task_combine: sum_t w[t] M[t] (t ascending) written into the network's padded
 * gradient buffer and read back leaf by leaf into out_dense[P]. */
int mtsac_set_pcgrad(mtsac_engine* h, int32_t on, int32_t cosine_sim_logs);
int mtsac_pcgrad_set_order(mtsac_engine* h, const int32_t* critic_perm, const int32_t* actor_perm);
int mtsac_pcgrad_get_order(mtsac_engine* h, int32_t* critic_perm, int32_t* actor_perm);
int mtsac_get_pcgrad_logs(mtsac_engine* h, float* out /* 10 */);
int mtsac_task_gram(mtsac_engine* h, int which, double* gram);
int mtsac_task_pcgrad_solve(mtsac_engine* h, int which, const int32_t* perm, int32_t cosine_sim_logs, float* w,
                            float* logs /* 6 */);
int mtsac_task_combine(mtsac_engine* h, int which, const float* w, float* out_dense);

/* ---- CAGrad (CAGradConfig on both optimizers, mtrl/config/optim.py and mtrl/optim/cagrad.py).
 * DESIGN.md section 11.  The same split-loss step as PCGrad's with another solve between the Gram matrix
 * and the combine: the per-task clip to norm 1, the scaling, num_iterations - 1 momentum-SGD steps on the
 * task weights (from zeros) and a final evaluation, softmax of the best iterate, the combine weights.
 * mtsac_set_cagrad: on = 1 makes mtsac_update / mtsac_update_many run the CAGrad step for BOTH networks.
 * The reference's values are c = 0.5, num_iterations = 21, learning_rate = 25 (50 from 50 tasks on),
 * momentum = 0.5.  Limits and error codes as mtsac_set_pcgrad (-95 sharded or use_task_weights, -22 above
 * 64 tasks, -12 out of memory, eager step: mtsac_enable_graph(1) returns -95 while on); -16 while PCGrad
 * is on (and mtsac_set_pcgrad(1) returns -16 while CAGrad is on); -22 for num_iterations < 1 or > 1024, a
 * non-finite or negative c, a non-finite learning_rate or momentum.  Log slots 2, 5, 7 as in the PCGrad
 * step.
 * mtsac_get_cagrad_logs: per network (critic, then actor) the CAGradState of the last step after
 * task_weights -- avg_grad_magnitude, avg_grad_magnitude_before_surgery, avg_cosine_similarity (NaN
 * without cosine_sim_logs), cagrad_objective -- then the T task_weights: out[2 * (4 + T)].
 * mtsac_task_cagrad_solve: the kernel alone, on the matrix mtsac_set_task_gradients / mtsac_task_gradients
 * left: Gram + solve from the start w0 (NULL: zeros): w[T] (the combine weights on the raw rows, for
 * mtsac_task_combine), task_weights[T], logs[6] (the four scalars above, the index of the best iterate,
 * |mean_t g_t|), obj_hist[num_iterations] (the objective at every evaluated iterate, fp64). */
int mtsac_set_cagrad(mtsac_engine* h, int32_t on, double c, int32_t num_iterations, double learning_rate,
                     double momentum, int32_t cosine_sim_logs);
int mtsac_get_cagrad_logs(mtsac_engine* h, float* out /* 2 * (4 + T) */);
int mtsac_task_cagrad_solve(mtsac_engine* h, int which, double c, int32_t num_iterations, double learning_rate,
                            double momentum, const double* w0, int32_t cosine_sim_logs, float* w,
                            float* task_weights, float* logs /* 6 */, double* obj_hist);

/* ---- GradNorm (GradNormConfig on both optimizers, mtrl/config/optim.py and mtrl/optim/gradnorm.py).
 * DESIGN.md section 12.  The same split-loss step with a third solve between the Gram matrix and the
 * combine.  It also consumes the per-task loss values and carries state from step to step: T task weights
 * (normalised to sum T), the latched first losses (+inf until then), and an inner [clip_by_global_norm +]
 * Adam on the weights.  Read literally, the reference's loss does not depend on the weights, so their
 * gradient is exactly zero: the weights stay the normalised initial_weights and the update is
 * sum_t w_t s_t g_t (a sum over the tasks, s_t the per-task clip to norm 1.0).  weighted_norms = 1 is the
 * form the reference has commented out (the task norms multiplied by the weights), where the weights move.
 * Arrays of two are indexed 0 critic, 1 actor.
 * mtsac_set_gradnorm: on = 1 makes mtsac_update / mtsac_update_many run the GradNorm step for BOTH networks
 * and (re-)initialises the state from initial_weights ([2][T], NULL: ones).  per_task_clip is
 * bool(GradNormConfig.max_grad_norm); inner_* are the gradnorm_optimizer's lr, eps and max_grad_norm
 * (negative: no clip).  Limits and error codes as mtsac_set_cagrad (-95 sharded or use_task_weights, -22
 * above 64 tasks, -12 out of memory, eager step: mtsac_enable_graph(1) returns -95 while on); -16 while
 * PCGrad or CAGrad is on (and their setters return -16 while GradNorm is on); -22 for non-finite values or
 * initial_weights that sum to zero.  Log slots 2, 5, 7 as in the PCGrad step.
 * mtsac_gradnorm_get_state / _set_state: one network's state (for a checkpoint, or an engine rebuilt at
 * another geometry); count is the inner Adam's.
 * mtsac_get_gradnorm_logs: per network (critic, then actor) the T task_weights, the T original_losses,
 * gradnorm_loss of the last step: out[2 * (2 T + 1)].
 * mtsac_get_gradnorm_task_losses: the per-task loss values the last step's solves read: out[2][T].
 * mtsac_task_gradnorm_solve: the kernel alone, on the matrix mtsac_set_task_gradients /
 * mtsac_task_gradients left, with the task losses and the state passed in: the state arrays and count are
 * read and overwritten with the new state; w[T] are the combine weights on the raw rows (for
 * mtsac_task_combine); logs[3] = gradnorm_loss, the sign margin min_t |d_t| / mean(n), |mean_t g_t|. */
int mtsac_set_gradnorm(mtsac_engine* h, int32_t on, double asymmetry, const int32_t* per_task_clip /* 2 */,
                       const double* inner_lr /* 2 */, const double* inner_eps /* 2 */,
                       const double* inner_max_grad_norm /* 2 */, const float* initial_weights /* [2][T] or NULL */,
                       int32_t weighted_norms);
int mtsac_gradnorm_get_state(mtsac_engine* h, int which, float* task_weights, float* original_losses, float* mu,
                             float* nu, int64_t* count);
int mtsac_gradnorm_set_state(mtsac_engine* h, int which, const float* task_weights, const float* original_losses,
                             const float* mu, const float* nu, int64_t count);
int mtsac_get_gradnorm_logs(mtsac_engine* h, float* out /* 2 * (2 T + 1) */);
int mtsac_get_gradnorm_task_losses(mtsac_engine* h, float* out /* 2 * T */);
int mtsac_task_gradnorm_solve(mtsac_engine* h, int which, const float* task_losses, double asymmetry,
                              int32_t per_task_clip, double inner_lr, double inner_eps, double inner_max_grad_norm,
                              int32_t weighted_norms, float* task_weights, float* original_losses, float* mu,
                              float* nu, int64_t* count, float* w, float* logs /* 3 */);

/* ---- network health metrics (MTSAC.get_metrics, mtsac.py; get_dormant_neuron_logs and compute_srank,
 * mtrl/monitoring/metrics.py).  DESIGN.md section 15.  Evaluation time: nothing is updated.
 * mtsac_network_metrics: the actor forward on batch->observations (only that field is read; the others may be
 * NULL), a = tanh(mu + sigma eps) with eps [B][A] injected or NULL (the device noise stream at the position
 * mtsac_task_gradients reads), the ONLINE critic's forward on (a, observations); then, for every trunk layer i
 * of every member e (the actor has one, the critic num_critics) and its post-ReLU output H [B][W] (the B = n T
 * real rows only):
 *   what bit 0  s_j = mean_b |H[b][j]|, the normalised scores s_j / (mean_j s_j + 1e-9) and the number of
 *               neurons whose normalised score is <= threshold (the reference's 0.1);
 *   what bit 1  the fp64 Gram matrix H^T H (W <= B) or H H^T (W > B), r x r with r = min(B, W): the squares of
 *               H's singular values are its eigenvalues (the host computes srank from them).
 * batch NULL samples on the device (advancing the index stream, as mtsac_task_gradients does); rows must be
 * interleaved i*T + t.  -95 on a task-sharded engine, -22 for what == 0, bits above 1 or a non-finite
 * threshold.  Works at every precision, action_dim and gradient-surgery mode; a captured step graph, the
 * parameters, the optimizer state and the logs stay as they are.  The trunk runs on fp32 operands as in the
 * rollout and mtsac_task_gradients passes (fp32 MFMA, or the on-the-fly 3-way bf16 split), so the GEMM error
 * bound is the one documented at enum mtsac_precision whatever the engine's precision.
 * which: 0 actor, 1 critic.  mtsac_get_network_scores: scores [E][D][W] (normalised), counts [E][D] of the
 * last call with bit 0; mtsac_network_gram_dim: r; mtsac_get_network_gram: one [r][r] matrix of the last call
 * with bit 1.  The scratch is allocated at the first call that needs it and freed with the engine.
 * mtsac_network_eigvals: the eigenvalues of the Grams of the last call with bit 1, solved on the device
 * (Householder reduction and bisection): lam [E][D][r] ascending, flags [E][D] (nonzero:
 * that Gram held a non-finite entry and its row of lam is NaN).  The solve runs in place: the Grams of `which`
 * are consumed, and mtsac_get_network_gram and a second mtsac_network_eigvals for it return -22 until the next
 * mtsac_network_metrics call with bit 1.  -22 without such a call, -95 on a task-sharded engine. */
int mtsac_network_metrics(mtsac_engine* h, const mtsac_batch* batch, const float* eps, int32_t what, float threshold);
int mtsac_get_network_scores(mtsac_engine* h, int which, float* scores, int32_t* counts);
int mtsac_network_gram_dim(const mtsac_engine* h, int which);
int mtsac_get_network_gram(mtsac_engine* h, int which, int32_t member, int32_t layer, double* gram);
int mtsac_network_eigvals(mtsac_engine* h, int which, double* lam, int32_t* flags);

#ifdef __cplusplus
}
#endif
#endif /* MTSAC_H_ */
