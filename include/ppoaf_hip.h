/*
 * ppoaf_hip.h -- C ABI of libppoaf_hip.so, the MI355X (gfx950) hot path that
 * stands in for LLNL/ppo_and_friends' rollout-buffer + PPO-update arithmetic.
 *
 * The reference is pure Python (no FFI of its own); every entry point below
 * replaces a chain of NumPy / PyTorch ops or a Python loop, cited per function
 * as /root/reference-relative file:line.  The Python host (ppo_and_friends_amd/)
 * binds these with ctypes; INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (torch tensor
 *     .data_ptr()); the caller owns the memory; nothing is allocated here except
 *     the small per-process scratch noted on individual calls;
 *   - the last argument is the hipStream_t to enqueue on (NULL = default
 *     stream); calls are asynchronous on that stream and never synchronise, so
 *     they are hipGraph-capturable;
 *   - return 0 on success, <0 on error (PPOAF_E_*); ppoaf_last_error() returns
 *     a thread-local message;
 *   - shapes are checked on the host before any launch; no kernel is launched
 *     with a shape it does not handle;
 *   - single Python thread per rank issues the calls; the library keeps no
 *     host threads.
 */
#ifndef PPOAF_HIP_H
#define PPOAF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ppoaf_stream_t;            /* hipStream_t */

#define PPOAF_OK            0
#define PPOAF_E_INVALID    -1            /* bad argument / unsupported shape   */
#define PPOAF_E_LAUNCH     -2            /* hipLaunch / runtime error          */

#define PPOAF_ABI_VERSION 7

int         ppoaf_abi_version(void);
const char* ppoaf_last_error(void);
/* Number of CUs of the current device (used by the host to size grids in tests). */
int         ppoaf_device_cu_count(void);

/* ------------------------------------------------------------------------ *
 * K1  GAE advantages + rewards-to-go
 * replaces EpisodeInfo.end_episode / compute_discounted_sums /
 *          _compute_gae_advantages   utils/episode_info.py:223-293,419-465
 * Numerics: delta = r + f64(fl32(gamma*V[t+1])) - V[t]; both scans accumulate
 * in float64 (the reference's accumulator under its pinned numpy<1.24), results
 * rounded once to float32 (PPODataset.build's float32 cast, :868-887).
 * ending_reward is clipped to [clip_lo, clip_hi] when has_clip (:450-454) and
 * rounded to float32 (:456-457); ending_value is NOT clipped (:410-411).
 * use_gae == 0  ->  advantages = rtg - V (:295-301).
 * ------------------------------------------------------------------------ */

/* Dense time-major rollout buffer [T,E] (E contiguous): the build's native
 * layout.  end_kind[t,e]: 0 = episode continues into t+1, 1 = terminal end
 * (ending value/reward 0, ppo.py:1818-1819), 2 = bootstrapped end (ending
 * value = boot_value[t,e], ending reward = boot_reward[t,e]; ppo.py:1932-1938).
 * Row T-1 must be non-zero everywhere (ppo.py:1870-1871) -- when end_kind is
 * NULL the trajectories are fixed-length: only row T-1 ends, bootstrapped, and
 * boot_value / boot_reward are [E] arrays.  Otherwise they are [T,E] and read
 * only where end_kind == 2. */
int ppoaf_gae_rtg_tmajor(const float* rewards, const float* values,
                         const float* boot_value, const float* boot_reward,
                         const int8_t* end_kind,
                         int32_t T, int64_t E,
                         double gamma, double lambd,
                         int has_clip, double clip_lo, double clip_hi,
                         int use_gae,
                         float* adv_out, float* rtg_out,
                         ppoaf_stream_t stream);

/* Same launch with the kernel's own begin / end stamped into two events (hipExtLaunchKernelGGL):
 * what bench.py uses for the roofline figure.  Events come from ppoaf_event_create(). */
int ppoaf_gae_rtg_tmajor_timed(const float* rewards, const float* values,
                               const float* boot_value, const float* boot_reward,
                               const int8_t* end_kind,
                               int32_t T, int64_t E,
                               double gamma, double lambd,
                               int has_clip, double clip_lo, double clip_hi,
                               int use_gae,
                               float* adv_out, float* rtg_out,
                               void* start_event, void* stop_event,
                               ppoaf_stream_t stream);
void* ppoaf_event_create(void);
int   ppoaf_event_destroy(void* event);
/* waits for `stop`, then *ms = time between the two stamps */
int   ppoaf_event_elapsed_ms(void* start_event, void* stop_event, float* ms);

/* Ragged trajectory list over a flat episode-major [N] layout (the layout
 * PPODataset.build produces, utils/episode_info.py:745-914): trajectory i
 * covers [traj_start[i], traj_start[i] + traj_len[i]).  Used for the
 * EpisodeInfo-level drop-in and PPODataset.recalculate_advantages (:721-743;
 * pass rtg_out = NULL there: rtg is not recomputed by the reference). */
int ppoaf_gae_rtg_traj(const float* rewards, const float* values,
                       const float* ending_value, const float* ending_reward,
                       const int64_t* traj_start, const int32_t* traj_len,
                       int64_t n_traj,
                       double gamma, double lambd,
                       int has_clip, double clip_lo, double clip_hi,
                       int use_gae,
                       float* adv_out, float* rtg_out,
                       ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K2+K3  mini-batch advantage normalisation + PPO loss, forward and backward
 * replaces PPO._ppo_batch_train  ppo.py:2325-2333 (normalise), 2352-2438 (loss)
 *
 * Inputs are length-B float32 streams.  adv is the RAW advantage; when
 * normalize_adv it is replaced by (adv-mean)/(unbiased_std+1e-8) (ppo.py:2326-2333).
 * Outputs:
 *   scalars[0] actor surrogate loss  mean(-min(surr1,surr2))        ppo.py:2392
 *   scalars[1] total actor loss = [0] - w_ent*mean(H) + kl_w*kl     ppo.py:2395-2405
 *   scalars[2] critic loss (MSE, or Huber(delta) if use_huber)      ppo.py:2416-2419
 *   scalars[3] mean entropy                                         ppo.py:2396
 *   scalars[4] kl = mean(old_logp - cur_logp)                       ppo.py:2358
 *   scalars[5] advantage mean, scalars[6] advantage unbiased std
 *   scalars[7] 1.0 if any ratio is NaN/Inf (ppo.py:2361), else 0.0
 *   d_logp[B], d_entropy[B]  = d scalars[1] / d cur_logp, / d entropy
 *   d_values[B]              = d scalars[2] / d values
 * The kl_loss_weight term carries no gradient (ppo.py:2403-2405 adds a Python
 * float).  The entropy term is skipped when entropy_weight == 0 (ppo.py:2395).
 * The vf_clip branch of the reference raises AttributeError (ppo.py:2432) and
 * is not reproduced.  Any gradient pointer may be NULL (forward only).
 * ------------------------------------------------------------------------ */
int ppoaf_ppo_loss_fwd_bwd(const float* cur_logp, const float* old_logp,
                           const float* adv, const float* entropy,
                           const float* values, const float* rtg,
                           int64_t B,
                           int normalize_adv, float surr_clip,
                           float entropy_weight, float kl_loss_weight,
                           int use_huber, float huber_delta,
                           float* scalars /* [8] */,
                           float* d_logp, float* d_entropy, float* d_values,
                           ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K4  mini-batch gather
 * replaces DataLoader(shuffle=True) + PPODataset.__getitem__ + default collate
 *          ppo.py:2181-2184,2292-2295; utils/episode_info.py:922-952
 * For b in [0,B): row = perm[b]; if row_map: row = row_map[row];
 *                 dst_f[b, :] = src_f[row, :]  for every field f.
 * row_map maps a position in the reference's flattened episode-major order to
 * the row of the time-major [T*E] buffer (NULL = identity).  Up to
 * PPOAF_MAX_GATHER_FIELDS fields per launch; row_bytes must be a multiple of 4.
 * ------------------------------------------------------------------------ */
#define PPOAF_MAX_GATHER_FIELDS 8
typedef struct {
    const void* src;        /* [n_rows, row_bytes] */
    void*       dst;        /* [B, row_bytes]      */
    int32_t     row_bytes;
    int32_t     _pad;
} ppoaf_gather_field_t;

int ppoaf_minibatch_gather(const ppoaf_gather_field_t* fields /* host array */,
                           int32_t n_fields,
                           const int64_t* perm, const int32_t* row_map,
                           int64_t n_rows, int64_t B,
                           ppoaf_stream_t stream);

/* Scatter of the freshly evaluated critic values back into the dataset
 * (ppo.py:2340  dataset.values[batch_idxs] = values.detach()). */
int ppoaf_scatter_rows_f32(const float* src /* [B] */, const int64_t* perm,
                           const int32_t* row_map, int64_t n_rows, int64_t B,
                           float* dst /* [n_rows] */, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K5  running mean / variance (value, observation and reward normalisers)
 * replaces RunningMeanStd.update/_integrate_batch_data  utils/stats.py:29-94
 *          RunningStatNormalizer.normalize/denormalize  utils/misc.py:84-128
 * State lives on the device: mean[W], var[W] float32, count[1] float64
 * (initialise mean 0, var 1, count 1e-4: stats.py:25-27).
 * ------------------------------------------------------------------------ */

/* moments_out[0] = n, [1..W] = batch mean, [1+W..2W] = batch M2 = sum (x-mean)^2,
 * all float64; data is [n, W] float32 row-major. */
int ppoaf_batch_moments(const float* data, int64_t n, int32_t W,
                        double* moments_out /* [1+2W] */, ppoaf_stream_t stream);

/* Merge R per-rank moment records (concatenated, [R, 1+2W]; R = 1 on a single
 * rank; more after an all-gather -- equal to the reference's allgather of the
 * raw data, stats.py:47-50) into one batch (Chan), then integrate that batch
 * into the running state exactly as stats.py:73-94 does. */
int ppoaf_running_moments_integrate(const double* moments, int32_t R, int32_t W,
                                    float* mean, float* var, double* count,
                                    ppoaf_stream_t stream);

/* out = (x - mean) / sqrt(var + eps)   misc.py:106-111 ; x is [n, W] */
int ppoaf_normalize(const float* x, int64_t n, int32_t W,
                    const float* mean, const float* var, float eps,
                    float clip_lo, float clip_hi, int has_clip,
                    float* out, ppoaf_stream_t stream);
/* out = mean + x * sqrt(var + eps)     misc.py:124-128 */
int ppoaf_denormalize(const float* x, int64_t n, int32_t W,
                      const float* mean, const float* var, float eps,
                      float* out, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K6  action distributions
 * replaces CategoricalDistribution / GaussianDistribution
 *          networks/distributions.py:199-269, 441-694 and
 *          PPOPolicy.get_rollout_actions / evaluate  policies/ppo_policy.py:729-794,891-952
 * Categorical(probs) semantics of torch.distributions: probs renormalised by
 * their sum, logits = log(clamp(probs, eps, 1-eps)) with eps = FLT_EPSILON.
 * ------------------------------------------------------------------------ */

/* Rollout: logits [n,K] -> softmax -> sample (Philox4x32-10 keyed by seed,
 * counter = offset + row) -> log-prob of the sample.  probs_out may be NULL. */
int ppoaf_categorical_sample(const float* logits, int64_t n, int32_t K,
                             uint64_t seed, uint64_t offset,
                             int64_t* action_out, float* logp_out,
                             float* probs_out, ppoaf_stream_t stream);

/* Update: logits [n,K], actions [n] -> logp[n], entropy[n] (+ probs for bwd). */
int ppoaf_categorical_eval_fwd(const float* logits, const int64_t* actions,
                               int64_t n, int32_t K,
                               float* logp_out, float* entropy_out,
                               float* probs_out, ppoaf_stream_t stream);
/* d_logits[n,K] from d_logp[n], d_entropy[n] (either may be NULL = zeros). */
int ppoaf_categorical_eval_bwd(const float* probs, const int64_t* actions,
                               const float* d_logp, const float* d_entropy,
                               int64_t n, int32_t K,
                               float* d_logits, ppoaf_stream_t stream);

/* Gaussian with tanh squashing (distributions.py:441-694):
 *   std = max(softplus(log_std), min_std)                         :514-516
 *   logp = sum_d clamp(N(mean,std).log_prob(x), -100, 100)
 *          - sum_d log(clamp(1 - tanh(x)^2, 1e-6, inf))            :551-558
 *   entropy = -logp(x := mean): PPOPolicy.evaluate asks for the entropy at the
 *             distribution's own mean                  ppo_policy.py:950, :672-694
 * mean, x: [n,D]; log_std: [D]. */
int ppoaf_gaussian_tanh_eval_fwd(const float* mean, const float* log_std,
                                 const float* x, int64_t n, int32_t D,
                                 float min_std,
                                 float* logp_out, float* entropy_out,
                                 ppoaf_stream_t stream);
/* d_mean[n,D], d_log_std[D] (the sum over all rows, in a fixed order: one launch, no memset, no atomics -- safe
 * inside a captured hipGraph) from d_logp[n] and d_entropy[n]. */
int ppoaf_gaussian_tanh_eval_bwd(const float* mean, const float* log_std,
                                 const float* x, const float* d_logp,
                                 const float* d_entropy, int64_t n, int32_t D,
                                 float min_std,
                                 float* d_mean, float* d_log_std,
                                 ppoaf_stream_t stream);
/* Rollout: raw = mean + std * N(0,1) (Philox), action = tanh(raw) rescaled to
 * [act_lo[d], act_hi[d]] per action dimension (device float32[D]; both NULL: the
 * unit box, no rescale) (:476-483, :580-609, :645-672), logp as above. */
int ppoaf_gaussian_tanh_sample(const float* mean, const float* log_std,
                               int64_t n, int32_t D, float min_std,
                               const float* act_lo, const float* act_hi,
                               uint64_t seed, uint64_t offset,
                               float* raw_out, float* action_out,
                               float* logp_out, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K11  flat-bucket gradient clip + Adam
 * replaces PPOPolicy.update_weights' clip_grad_norm_ + Adam.step
 *          policies/ppo_policy.py:1037-1042,1050-1055 (Adam eps 1e-5 :336-339)
 *          and the 1/num_procs of mpi_avg  utils/mpi_utils.py:86
 * params/grads/exp_avg/exp_avg_sq are flat float32 buckets of n elements.
 * grad_scale multiplies the gradient first (1/world_size after a SUM
 * all-reduce).  max_norm <= 0 disables clipping; otherwise
 * coef = min(1, max_norm / (||grad_scale*g||_2 + 1e-6)) as torch does.
 * step_count is the 1-based Adam step kept on the device (int64[1],
 * incremented by the call) so the launch is graph-replayable.
 * norm_scratch: float64[PPOAF_NORM_SCRATCH_DOUBLES] device scratch owned by the caller: [0] receives the squared
 * norm, [2..] per-workgroup partials.  No atomics anywhere: the partials are added in a fixed association, so the
 * clip coefficient is bitwise the same in every run and on every rank of a DD-PPO job.
 * ------------------------------------------------------------------------ */
#define PPOAF_NORM_SCRATCH_DOUBLES 66
int ppoaf_clip_adam_step(float* params, const float* grads,
                         float* exp_avg, float* exp_avg_sq, int64_t n,
                         int64_t* step_count, const float* lr /* device [1] */,
                         float beta1, float beta2, float eps,
                         float grad_scale, float max_norm,
                         double* norm_scratch, float* grad_norm_out /* NULL ok */,
                         ppoaf_stream_t stream);
/* The Adam half alone: step_count has been advanced for this step and ||grad_scale * grads||^2 is known -- as
 * norm_scratch[0] (n_norm_partials = 0: e.g. ppoaf_peer_exchange_allreduce's norm_out), or as n_norm_partials
 * per-workgroup partials norm_scratch[2 ..] left by a producer kernel (K15's reduce with fuse_norm), which are added
 * in a fixed association here (and the sum stored to norm_scratch[0]). */
int ppoaf_adam_step_prenormed(float* params, const float* grads,
                              float* exp_avg, float* exp_avg_sq, int64_t n,
                              const int64_t* step_count, const float* lr /* device [1] */,
                              float beta1, float beta2, float eps,
                              float grad_scale, float max_norm,
                              double* norm_scratch, int32_t n_norm_partials, float* grad_norm_out /* NULL ok */,
                              ppoaf_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K12  fused PPO mini-batch update for MLP actor/critic (discrete or
 *      tanh-Gaussian head): the whole body of one iteration of
 *      PPO._ppo_batch_train  ppo.py:2292-2469  in three launches
 *
 *   ppoaf_ppo_update_fwd_bwd : grid (ceil(B/16), 2 networks).  Each workgroup
 *        gathers its 16 rows through perm / row_map (K4), the critic side
 *        integrates this mini-batch's value-normaliser record and normalises
 *        rewards-to-go (K5, ppo.py:2299-2303), the actor side normalises the
 *        advantages over the whole mini-batch (K2, :2325-2333); forward through
 *        the MLP (hidden layers on f32 MFMA 16x16x4, exact fmaf chains),
 *        distribution log-prob / entropy (K6), loss terms (K3), dataset.values
 *        write-back (:2340), backward through the MLP; weight-gradient partials
 *        go to this workgroup's slab with plain stores (no atomics: the sum
 *        order is fixed, results are bitwise reproducible).
 *   ppoaf_ppo_update_reduce  : slabs -> flat gradient bucket (fixed order),
 *        per-workgroup loss partials -> running totals; optionally the squared
 *        gradient norms (single rank).  An all-reduce of the bucket goes
 *        between this and the next call on multi-rank runs.
 *   ppoaf_ppo_update_adam    : [norms if not done] clip + Adam for both
 *        networks (ppo_policy.py:1037-1055), advances the mini-batch cursor.
 *        compute_norms 0: the reduce launch (compute_norms = 1 there) left the
 *        per-workgroup squared-norm partials in norm_scratch[6 ..]; 1: compute
 *        those partials now (after an all-reduce of the bucket); 2:
 *        norm_scratch[0..1] already hold the two squared norms
 *        (ppoaf_peer_exchange_allreduce's norm_out).  Partials are added in a
 *        fixed association -- no atomics: the clip coefficients are bitwise the
 *        same in every run and on every rank.
 *
 * All three read the mini-batch index from a device cursor, so one captured
 * hipGraph of N repetitions walks N consecutive mini-batches of the epoch.
 * Network parameters are the flat bucket of nn.Linear tensors in module order
 * (weight [out,in] row-major then bias, each padded to 4 floats), hidden
 * layers of equal width H per network; instantiated (actor, critic) widths:
 * (32,32) (64,64) (128,128) (256,256) (128,256) (64,128) (64,256) (32,256)
 * (32,64); depth >= 1.  One list names them for every launch of K6+K7 and K12
 * (csrc/ppo_update_dev.hpp: PPOAF_WIDTH_PAIRS); a critic narrower than its
 * actor and 512-wide networks are refused.
 * out_dim: 1 .. 8.  The 256-wide actor of the wide pair (256, 512) takes
 * 9 .. 24 outputs under PPOAF_HEAD_CATEGORICAL and PPOAF_HEAD_GAUSSIAN (the
 * wide heads: Discrete(18), Box(17)) in ppoaf_policy_step, its block form and
 * ppoaf_ppo_update_*, on kernels of their own that the library picks from
 * out_dim (csrc/policy_wide_heads.hip, csrc/ppo_update_wide_heads.hip); a
 * launch with out_dim <= 8 runs the kernel it always ran.  The two other
 * heads, every other pair and out_dim > 24 are refused by name.
 * ------------------------------------------------------------------------ */
#define PPOAF_ACT_RELU        0
#define PPOAF_ACT_LEAKY_RELU  1      /* negative slope 0.01 (nn.LeakyReLU default) */
#define PPOAF_ACT_TANH        2
#define PPOAF_HEAD_CATEGORICAL 0       /* Discrete: softmax -> Categorical, networks/distributions.py:199-269, :1043-1045 */
#define PPOAF_HEAD_GAUSSIAN    1       /* Box: tanh-Gaussian with a learned log_std, :441-694 */
/* MultiDiscrete (:272-438, output function :1047-1064): actor.out_dim = the sum of the slice table (n_action_slices,
 * action_slices[] at the end of the args structs); per slice softmax -> Categorical(probs); log-prob and entropy summed
 * over the slices.  Raw actions int64 [rows, n_action_slices]. */
#define PPOAF_HEAD_MULTI_CATEGORICAL 2
/* MultiBinary (:134-196, output function sigmoid :1111-1113): one bit per actor output, torch Bernoulli(probs =
 * sigmoid(z)) with its eps clamp; log-prob and entropy summed over the bits.  Raw actions float32 [rows, out_dim], 0 / 1. */
#define PPOAF_HEAD_BERNOULLI   3
#define PPOAF_UPDATE_ROWS_PER_WG 16

typedef struct {
    int32_t in_dim, hidden, depth, out_dim;   /* depth = number of hidden layers */
    int32_t activation, _pad;
    int64_t offset;        /* first float of this network inside the policy bucket */
    int64_t size;          /* floats of this network's bucket (incl. padding + log_std) */
    int64_t log_std_offset;/* actor, Gaussian head: offset of log_std [out_dim] inside the bucket, else -1 */
} ppoaf_mlp_desc_t;

typedef struct {
    ppoaf_mlp_desc_t actor, critic;
    /* parameters / optimiser state: one bucket, actor then critic */
    float* params; float* grads; float* exp_avg; float* exp_avg_sq;
    float* slabs;                 /* [n_wg, bucket_total] gradient partials               */
    int64_t bucket_total;
    int64_t* step_counts;         /* [2] Adam steps (actor, critic), incremented per call  */
    const float* lr;              /* [1] device                                            */
    double* norm_scratch;         /* [6 + 2 * ceil(bucket_total / 1024)]: squared norms (2) + Adam bias corrections (4)
                                   * + per-workgroup squared-norm partials (actor, critic) of the reduce / norm pass */
    float beta1, beta2, adam_eps, grad_scale, max_norm; int32_t head_kind;
    /* rollout buffer (time-major rows) */
    const float* obs; const float* critic_obs; const void* raw_actions;  /* int64 [n,1] / [n,D] or f32 [n,D] (head_kind) */
    const float* advantages; const float* old_log_probs; const float* rewards_to_go;
    float* values;                /* write-back target                                     */
    const int64_t* perm; const int32_t* row_map; int64_t n_rows;
    int64_t* cursor;              /* [1] mini-batch index within the epoch                 */
    int64_t B;                    /* rows of this mini-batch (<= batch capacity)           */
    int64_t batch_stride;         /* perm offset of mini-batch k = k * batch_stride        */
    /* value normaliser: double-buffered state (slot = cursor & 1), records [n_batches, R, 3] */
    int32_t normalize_values, n_ranks;
    float* vn_mean; float* vn_var; double* vn_count;    /* [2] each */
    const double* vn_records;
    /* advantage normalisation (ppo.py:2326-2333): (n, mean, M2) of the raw advantages of every
     * mini-batch of the epoch, [n_batches, 3] from ppoaf_minibatch_moments (rank-local) */
    const double* adv_records;
    /* loss */
    int32_t normalize_adv, use_huber;
    float surr_clip, entropy_weight, kl_loss_weight, huber_delta, min_std;
    /* 1: obs / critic_obs / raw_actions / advantages / old_log_probs / rewards_to_go are per-epoch
     * tables already in shuffled order (entry i belongs to perm[i]), so a mini-batch reads
     * [k * batch_stride, +B) directly -- no index -> data dependent load; `values` is still
     * written through perm / row_map.  0: they are the rollout buffer's rows. */
    int32_t inputs_in_batch_order;
    float* loss_partials;         /* [2, n_wg, 8]                                          */
    double* totals;               /* [9] sums of the 8 loss scalars + mini-batch count     */
    /* mini-batch index = *cursor + mb_offset; the Adam launch adds cursor_advance to *cursor.
     * Eager use: (0, 1).  A captured chain of n mini-batches bakes mb_offset = 0..n-1 into its nodes
     * and advances the cursor once, by n, in the last one: the cursor word is then rewritten once per
     * chain instead of once per mini-batch, so all but the first read of it hit the reader's L2. */
    int64_t mb_offset, cursor_advance;
    /* split-wgrad chain (NULL: weight-gradient slabs + ppoaf_ppo_update_reduce).  With a workspace of
     * ppoaf_ppo_update_split_workspace_bytes() bytes (256-byte aligned) fwd_bwd computes no hidden-layer weight gradient:
     * every workgroup publishes its 16 rows of the inputs, hidden activations and dLoss/dz of the mini-batch there, and
     * ppoaf_ppo_update_wgrad forms the complete gradients from those panels (then ppoaf_ppo_update_adam, compute_norms 3).
     * Per network: hidden activations and dLoss/dz [depth][Bp][hidden], the output layer's partials and the gathered input
     * rows [Bp][64 | 128] (Bp = B rounded up to 64; 128: a wide pair's network with more than 64 inputs, PPOAF_SPLIT_WIDE_INPUTS;
     * [Bp][256 | 512] for one with more than 128 | 256 inputs, PPOAF_SPLIT_WIDE_SHAPES). */
    void* split_workspace; int64_t split_workspace_bytes;
    /* 0: fwd_bwd's workgroups use every XCD (actor on 0-3, critic on 4-7; default).  1 / 2: they sit on XCDs 0-3 / 4-7 only
     * (actor on the half's first two XCDs, critic on the other two; the launch is twice as wide and the workgroups
     * dispatched to the other half return at once): when another update chain (K14: ppoaf_icm_update_args_t.xcd_half)
     * runs on a second stream, each keeps its weights and panels in its own four L2s -- C3: +2 % env-steps/s; alone the
     * confinement costs 1 % (C2).  Placement only changes speed. */
    int32_t xcd_half;
    /* ABI 6.  Options of the split-wgrad chain, a bit set (the field keeps the name of its first option; 0: none).
     * PPOAF_SPLIT_ROW_PAIRS (1; with split_workspace only, ignored otherwise): the 16-row tiles of a 256-wide network of depth 2 .. 4 run on
     * PAIRS of workgroups (a 32-, 64- or 128-wide actor beside such a critic keeps one workgroup per tile; a 256-wide actor
     * beside it must be of depth 2 .. 4 itself, else neither network runs in pairs) that split every hidden layer pass by output columns and exchange the halves through tagged
     * records behind the panels of split_workspace (csrc/ppo_update_rowpair.hpp) -- ppoaf_ppo_update_split_workspace_bytes()
     * then includes the record region.  Results are BITWISE those of row_pairs = 0.  The tag is the mini-batch index + 1:
     * the caller zeroes split_workspace before the first launch and whenever mini-batch indices restart (every epoch).
     * The region's first 32-bit word (byte offset ppoaf_ppo_update_row_pairs_error_offset()) is non-zero after a launch in
     * which a partner did not answer within 2 s; that launch's results are invalid.
     * PPOAF_SPLIT_WIDE_INPUTS (2; added within ABI 7, read by every entry point, ppoaf_ppo_update_check included): an opt-in
     * for the wide pair (actor 256, critic 512), which runs the split-wgrad chain only.  Without it every check, message and
     * workspace size is what it was (in_dim <= 64).  With it the pair takes in_dim <= 128 per network: the layer-0 panel of
     * a network with 64 < in_dim <= 128 has a row stride of 128 floats instead of 64 (ppoaf_ppo_update_split_workspace_bytes()
     * counts it); a network with in_dim <= 64 keeps the stride of 64, and its results are bitwise those without the bit.
     * Every other pair ignores the bit: with a split workspace it keeps in_dim <= 64 (wider inputs run its slab chain).
     * PPOAF_SPLIT_WIDE_SHAPES (4; added within ABI 7, read by every entry point; implies PPOAF_SPLIT_WIDE_INPUTS): a second
     * opt-in for the wide pair.  With it the pair takes in_dim <= 512 per network, as far as each row-tile body's LDS goes
     * (the 256-wide actor: 512 inputs at depth 1 and 2, 432 at depth 3, 160 at depth 4, none deeper; the 512-wide critic:
     * 512 at every depth 1 .. 7; a refusal for LDS names LDS), and B <= 1024.  The layer-0 panel's row stride is the
     * smallest of 64, 128, 256, 512 floats that holds the network's in_dim; Bp goes up to 1024.  ppoaf_ppo_update_wgrad takes
     * a mini-batch of more than 512 rows in two passes of 32 chunks of 16 rows over the same accumulators.  Inside the
     * limits of PPOAF_SPLIT_WIDE_INPUTS every size and result is bitwise what that bit alone gives.  Every other pair
     * ignores the bit, as it ignores the other.  Bits from 8 up are refused. */
#define PPOAF_SPLIT_ROW_PAIRS   1
#define PPOAF_SPLIT_WIDE_INPUTS 2
#define PPOAF_SPLIT_WIDE_SHAPES 4
    int32_t row_pairs;
    /* the slice table of PPOAF_HEAD_MULTI_CATEGORICAL: classes per action dimension, in order, summing to actor.out_dim.
     * Read only for that head kind (appended: every field above keeps its offset). */
    int32_t n_action_slices;
    int32_t action_slices[8];
} ppoaf_ppo_update_args_t;

int ppoaf_ppo_update_fwd_bwd(const ppoaf_ppo_update_args_t* args, ppoaf_stream_t stream);
/* same launch with the kernel's own begin / end stamped into two events (as ppoaf_gae_rtg_tmajor_timed) */
int ppoaf_ppo_update_fwd_bwd_timed(const ppoaf_ppo_update_args_t* args, void* start_event, void* stop_event,
                                   ppoaf_stream_t stream);
/* Host-only query (added within ABI 7: no field or call changed), nothing is launched and no pointer of args is read:
 * PPOAF_OK when fwd_bwd accepts these shapes (layer tables, bucket, head, batch size, the row-tile body's LDS, the
 * instantiated width pairs: the nine listed above ppoaf_mlp_desc_t, for every depth and in_dim whose row tile fits the LDS
 * of the wider network), else PPOAF_E_INVALID with the launch's own message in ppoaf_last_error().  The host
 * driver's scope test (fused_update.py: FusedPolicyUpdate.unsupported_reason) asks it. */
int ppoaf_ppo_update_check(const ppoaf_ppo_update_args_t* args);
int ppoaf_ppo_update_reduce(const ppoaf_ppo_update_args_t* args, int compute_norms, ppoaf_stream_t stream);
/* Split-wgrad chain: fwd_bwd (args->split_workspace set) -> ppoaf_ppo_update_wgrad -> ppoaf_ppo_update_adam(compute_norms 3).
 * The weight gradients of ppo.py:2443 (loss.backward()) are formed ONCE per mini-batch over all B rows -- one workgroup
 * per 16 x 16 tile of dW_l = dz_l^T h_{l-1} on f32 MFMA with K = B, db_l as column sums of dz_l, the output layer's
 * per-block partials folded in block order -- instead of 16-row partials written to B/16 slabs of the whole bucket and
 * summed by ppoaf_ppo_update_reduce: 8.7 MB of slab traffic per mini-batch at C2 become 1.6 MB of panels.  The same
 * launch folds the loss partials into totals, advances the step counters and leaves one pair of squared-norm partials
 * per workgroup in norm_scratch[6 ..] (needs 6 + 2 * ppoaf_ppo_update_split_blocks(args) doubles).  Sums run in MFMA K
 * order: float32-rounding-level differences from the slab chain, bitwise reproducible run to run. */
int ppoaf_ppo_update_split_workspace_bytes(const ppoaf_ppo_update_args_t* args, int64_t* bytes_out);
int ppoaf_ppo_update_split_blocks(const ppoaf_ppo_update_args_t* args);
/* byte offset of the row-pair error word inside split_workspace; -1 in *offset_out when args (row_pairs, shapes) select no pairs */
int ppoaf_ppo_update_row_pairs_error_offset(const ppoaf_ppo_update_args_t* args, int64_t* offset_out);
/* Which form of the fwd_bwd kernel ppoaf_ppo_update_fwd_bwd launches for these args (added within ABI 7; pure host, no pointer
 * of args is followed): *form_out = 1 for the lean kernel (csrc/ppo_update_lean.hip: the row-tile body compiled for one
 * activation and one head), 0 for the general one.  Lean needs ALL of: split_workspace set and no row pairs selected, both
 * networks of depth 3, inputs_in_batch_order, no row_map, actor.activation == critic.activation, head_kind Categorical or
 * Gaussian, hidden widths 32/32, 64/64, 128/128 or 64/128.  Results are BITWISE the general kernel's (the same expressions in
 * the same order: the forward and backward of PPO._ppo_batch_train, ppo.py:2292-2469). */
int ppoaf_ppo_update_fwd_bwd_form(const ppoaf_ppo_update_args_t* args, int32_t* form_out);
int ppoaf_ppo_update_wgrad(const ppoaf_ppo_update_args_t* args, ppoaf_stream_t stream);
/* Fused tail of the split-wgrad chain (ABI 5; csrc/ppo_update_tail.hip): fwd_bwd (args->split_workspace set) ->
 * ppoaf_ppo_update_wgrad_adam -- TWO launches per mini-batch.  Everything from loss.backward()'s weight gradients to
 * optimizer.step() (ppo.py:2443-2444, ppo_policy.py:1032-1055: backward, clip_grad_norm_, Adam, both networks) in one
 * launch: a workgroup forms one 16 x 32 piece of a layer's dW over all B rows (ppoaf_ppo_update_wgrad's jobs, bit for bit),
 * publishes its squared-norm partial as one tagged 16-byte record, waits for the records of all workgroups, and applies
 * clip + Adam to exactly its elements (their optimiser state was requested beside the MFMA operands).  Parameters, moments,
 * gradient bucket, totals, step counters and cursor end BITWISE as after ppoaf_ppo_update_wgrad + ppoaf_ppo_update_adam(3).
 * ctl: ppoaf_ppo_update_tail_ctl_bytes() bytes of device memory, 64-byte aligned, zeroed ONCE by the caller and then
 * kept across launches (it carries the launch tag); its third 32-bit word is non-zero after a launch in which a wait
 * ran out of wait_seconds (the workgroups were not all resident: the results of that launch are then invalid and later
 * launches do not wait again).  All 8 * per_xcd + 1 workgroups must fit on the device together (checked). */
int ppoaf_ppo_update_tail_ctl_bytes(const ppoaf_ppo_update_args_t* args, int64_t* bytes_out);
int ppoaf_ppo_update_wgrad_adam(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds, ppoaf_stream_t stream);
/* same launch with the kernel's own begin / end stamped into two events */
int ppoaf_ppo_update_wgrad_adam_timed(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds,
                                      void* start_event, void* stop_event, ppoaf_stream_t stream);
int ppoaf_ppo_update_adam(const ppoaf_ppo_update_args_t* args, int compute_norms, ppoaf_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K6+K7  one rollout step for all E envs of the rank in one launch
 * replaces PPOPolicy.get_rollout_actions            policies/ppo_policy.py:729-794
 *          PPO.get_policy_values + denormalisation  ppo.py:1030-1075, utils/misc.py:113-128
 *          the per-env EpisodeInfo.add_info calls   policies/ppo_policy.py:638-651
 * Actor and critic MLP forward (same tile code as the update kernel), sampling
 * (Philox4x32-10, counter = offset + env), log-prob, value (denormalised with the
 * running stats when normalize_values), written straight into row t of the
 * rollout buffer.  obs / critic_obs: [E, in_dim] float32; outputs are the row-t
 * slices of the buffer ([E,1] int64 actions for the categorical head, [E,D]
 * float32 for the Gaussian head, [E,D] int64 for the multi-categorical head --
 * slice j of env e samples with counter offset + j * E + e --, [E,n] float32
 * 0 / 1 for the Bernoulli head: bit d = u < sigmoid(z_d), u from counter offset + e,
 * subsequence d / 4).  *_copy_out (optional) receive the
 * observation rows.  Network descriptors as for K12.
 * ------------------------------------------------------------------------ */
typedef struct {
    ppoaf_mlp_desc_t actor, critic;
    const float* params;
    const float* obs; const float* critic_obs; int64_t E;
    int32_t head_kind; float min_std;
    const float* act_lo; const float* act_hi;   /* Gaussian head: bounds per action dimension (device float32[D]); both NULL = [-1,1] */
    const void* forced_raw_action;              /* NULL: sample.  Else the raw actions to log instead of sampling
                                                   ([E] int64 / [E,D] float32): replay of a recorded rollout */
    uint64_t seed, offset;
    int32_t normalize_values, _pad;
    const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out; float* value_out;
    float* obs_copy_out; float* critic_obs_copy_out;
    int32_t n_action_slices;                    /* PPOAF_HEAD_MULTI_CATEGORICAL only, as in ppoaf_ppo_update_args_t */
    int32_t action_slices[8];
} ppoaf_policy_step_args_t;

int ppoaf_policy_step(const ppoaf_policy_step_args_t* args, ppoaf_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K19  one evaluation step for all E rows in one launch (actor only)
 * replaces PPOPolicy.get_inference_actions          policies/ppo_policy.py:796-889
 *          (under PPO.get_inference_actions         ppo.py:896-1028, the step of testing.py:8-175)
 *          refine_prediction of the distributions   networks/distributions.py:177-196 (Bernoulli),
 *                                                   :262-263 (categorical), :404-436 (multi-categorical),
 *                                                   :580-581,611-631 (Gaussian: tanh + distribution_min/max rescale)
 * Actor MLP forward (the tile code K6 runs: csrc/mlp_device.hpp, mlp_rows_forward) -> head -> the ENVIRONMENT
 * action of every row.  ceil(E/16) workgroups of 512 threads.  obs: [E, in_dim] float32.  action_out in K6's
 * layouts: [E] int64 (categorical), [E,D] float32 (Gaussian), [E,D] int64 (multi-categorical), [E,n] float32 0 / 1
 * (Bernoulli).  mode:
 *   PPOAF_INFER_SAMPLE         K6's sampling with K6's Philox counters: for equal (obs, params, seed, offset) the
 *                              action is bitwise ppoaf_policy_step's action_out
 *   PPOAF_INFER_DETERMINISTIC  argmax (lowest index on an exact tie), argmax per slice, z >= 0 per bit, tanh(mean)
 *                              rescaled into [act_lo, act_hi]; seed / offset are not read
 * No log-prob, no value, no observation copies.  Shapes as K6: hidden width 32 / 64 / 128 / 256, out_dim <= 8; a
 * 256-wide actor takes out_dim 9 .. 24 under the categorical and the Gaussian head (the wide heads, a kernel of their
 * own: csrc/policy_wide_heads.hip; no critic here, so no pair is asked for).
 * ------------------------------------------------------------------------ */
#define PPOAF_INFER_SAMPLE        0
#define PPOAF_INFER_DETERMINISTIC 1

typedef struct {
    ppoaf_mlp_desc_t actor;
    const float* params;
    const float* obs; int64_t E;
    int32_t head_kind; int32_t mode;
    float min_std;
    int32_t n_action_slices;                    /* PPOAF_HEAD_MULTI_CATEGORICAL only, as in ppoaf_policy_step_args_t */
    int32_t action_slices[8];
    const float* act_lo; const float* act_hi;   /* Gaussian head: bounds per action dimension; both NULL = [-1,1] */
    uint64_t seed, offset;
    void* action_out;
} ppoaf_policy_infer_args_t;

int ppoaf_policy_infer(const ppoaf_policy_infer_args_t* args, ppoaf_stream_t stream);

/* Score bookkeeping of an evaluation (testing.py:59-112) for E environments in parallel, one small launch per env
 * step, nothing read by the host.  Row e owes quota[e] episodes (N // E + (e < N % E) of N test runs: "the first N
 * to finish" would be the SHORTEST episodes).  While count[e] < quota[e] the row adds score[e] (float32: the natural
 * reward when the env reports one, else the reward, testing.py:88-91) to run_score[e] and 1 to run_len[e]; where
 * done[e] (terminated | truncated, one byte per row) it then folds the episode into count / sum / min / max / steps,
 * clears the running pair and takes 1 off *remaining (one atomic add per finishing row).  A row that has met its quota
 * is left alone, so surplus steps change nothing.  Sums are float64 adds in step order.  The caller initialises
 * run_score = sum = 0, run_len = count = steps = 0, min = +inf, max = -inf, *remaining = N. */
typedef struct {
    const float* score; const uint8_t* done; const int32_t* quota; int64_t E;
    double* run_score; int64_t* run_len;
    int64_t* count; double* sum; double* min; double* max; int64_t* steps;
    int32_t* remaining;
} ppoaf_eval_scores_args_t;

int ppoaf_eval_scores_step(const ppoaf_eval_scores_args_t* args, ppoaf_stream_t stream);

/* The score books of a multi-agent evaluation (testing.py:59-112, the per-agent and per-policy sums of :93-98) in ONE
 * launch per env step instead of one ppoaf_eval_scores_step per agent and one more per agent for its policy's book.
 * score: [num_agents, E] float32, agent-major (what the env hands over); done: [E]; quota: [E], shared by every book.
 * Book b keeps its own rows of the [n_books, E] state arrays and its own remaining[b], and sums the agents whose bit is
 * set in book_mask[b] (bit a = agent a, num_agents <= 16, n_books <= 32):
 *   one bit     an agent's book: exactly the rule of ppoaf_eval_scores_step on score[a]
 *   more bits   a policy's book: exactly the chain of ppoaf_eval_scores_step calls it replaces -- the agents of the mask
 *               in ascending order, run_score += score[a][e] in float64 agent by agent, run_len + 1 PER AGENT, and the
 *               episode closes (done[e]) with the last agent of the mask
 * Results are bitwise those of the chain.  The caller initialises every book as ppoaf_eval_scores_step asks. */
typedef struct {
    const float* score; const uint8_t* done; const int32_t* quota; int64_t E;
    int32_t num_agents; int32_t n_books;
    int32_t book_mask[32];
    double* run_score; int64_t* run_len;
    int64_t* count; double* sum; double* min; double* max; int64_t* steps;
    int32_t* remaining;
} ppoaf_eval_books_args_t;

int ppoaf_eval_scores_step_books(const ppoaf_eval_books_args_t* args, ppoaf_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K8  ICM forward-model loss and intrinsic reward
 * replaces the tail of ICM.forward  networks/ppo_networks/icm.py:421-430
 *   intr[i]  = (reward_scale / 2) * sum_d (pred[i,d] - enc2[i,d])^2
 *   f_loss   = 0.5 * mean((pred - enc2)^2)
 * pred, enc2: [n, D] float32; rowsum_scratch: float32[n] owned by the caller;
 * intr_out / f_loss_out may be NULL.  bwd: d_pred = grad_f_loss * (pred-enc2)/(n*D),
 * d_enc2 = -d_pred (NULL to skip); grad_f_loss is a device scalar.
 * ------------------------------------------------------------------------ */
int ppoaf_icm_forward_loss_fwd(const float* pred, const float* enc2, int64_t n, int32_t D,
                               float reward_scale, float* rowsum_scratch, float* intr_out,
                               float* f_loss_out, ppoaf_stream_t stream);
int ppoaf_icm_forward_loss_bwd(const float* pred, const float* enc2, int64_t n, int32_t D,
                               const float* grad_f_loss, float* d_pred, float* d_enc2,
                               ppoaf_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K9  multi-agent-transformer attention core (f32 MFMA)
 * replaces the middle of SelfAttention.forward  networks/attention.py:94-103
 *   att = softmax(q k^T / sqrt(D) [causal mask]);  y = att v
 * q, k, v, y, dy, dq, dk, dv: [n_seq, L, D] float32 contiguous (heads folded into
 * n_seq), L <= 16 agents, D a multiple of 16; probs: [n_seq, L, L] (saved by fwd,
 * consumed by bwd).  floor(16/L) sequences are packed per 16-row MFMA tile.
 * ------------------------------------------------------------------------ */
int ppoaf_mat_attention_fwd(const float* q, const float* k, const float* v, int64_t n_seq,
                            int32_t L, int32_t D, int masked, float* y_out, float* probs_out,
                            ppoaf_stream_t stream);
int ppoaf_mat_attention_bwd(const float* q, const float* k, const float* v, const float* probs,
                            const float* dy, int64_t n_seq, int32_t L, int32_t D,
                            float* dq, float* dk, float* dv, ppoaf_stream_t stream);

/* (n, mean, M2) float64 records of the rewards-to-go of every mini-batch of an
 * epoch: records[k] covers perm[k*B : min((k+1)*B, n_perm)]  (ppo.py:2299-2303,
 * utils/stats.py:52-54 batched).  One workgroup per mini-batch. */
int ppoaf_minibatch_moments(const float* data, const int64_t* perm, const int32_t* row_map,
                            int64_t n_perm, int64_t B, double* records /* [ceil(n/B), 3] */,
                            ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K13  environment filters: running observation / reward normalisation and clipping
 * replaces ObservationNormalizer.step/reset        environments/filter_wrappers.py:155-268
 *          RewardNormalizer.step                   environments/filter_wrappers.py:388-458
 *          ObservationClipper / RewardClipper      environments/filter_wrappers.py:583-719
 * in the wiring order of wrapper_utils.py:81-111 (normalise, then clip).
 *
 * One env step of G agents x n envs (rows agent-major: group g owns rows [g*n, (g+1)*n)).
 * Two launches: `moments` reduces this rank's batch to a float64 record, the records of the
 * R ranks are all-gathered by the caller (R = 1: pass the record itself), `apply` merges
 * them into the running state and writes the filtered outputs.
 *
 * Record layout (float64, PPOAF_ENV_FILTER_RECORD_LEN(G, W_o, W_c, has_reward) values):
 *   [0] n | obs mean[G*W_o] | obs M2[G*W_o] | critic mean[G*W_c] | critic M2[G*W_c]
 *       | reward S1[G] | reward S2[G]
 * Observation stats are per (agent, feature): mean/var float32, count float64 (one copy per
 * column so no column races on it; initialise 0 / 1 / 1e-4, stats.py:25-27).
 * Reward stats per agent are float64 (the reference's become float64 on the first update).
 * The reference updates the reward stats n times per step, once after each env's running reward
 * is advanced, each time with the whole half-updated vector (filter_wrappers.py:412-418); the
 * n Chan merges equal one merge of the pooled n*n values, which is what S1/S2 carry:
 *   S1 = sum_i (n-i)(new_i - m) + i (old_i - m),  S2 likewise with squares, m = running mean.
 * A NULL filter pointer skips that stream.
 * ------------------------------------------------------------------------ */
typedef struct {
    const float* x;        /* [G, n, W] raw */
    float*       out;      /* [G, n, W] filtered (may alias x) */
    float*       mean;     /* [G, W] */
    float*       var;      /* [G, W] */
    double*      count;    /* [G, W] */
    int32_t      W;
    int32_t      normalize;  /* 0: clip only (mean/var/count may be NULL) */
    int32_t      update;     /* integrate this step into the running stats */
    int32_t      has_clip;
    float        clip_lo, clip_hi;
    float        eps;        /* 1e-8 */
} ppoaf_obs_filter_t;

typedef struct {
    const float*   reward;          /* [G, n] raw */
    const uint8_t* done;            /* [G, n] terminated */
    const uint8_t* done2;           /* [G, n] truncated, OR-ed with `done`; may be NULL */
    float*         out;             /* [G, n] */
    double*        running_reward;  /* [G, n] discounted running reward (state) */
    double*        mean;            /* [G] */
    double*        var;             /* [G] */
    double*        count;           /* [G] */
    int32_t        normalize;       /* 0: clip only (state pointers may be NULL) */
    int32_t        update;
    int32_t        has_clip;
    float          clip_lo, clip_hi;
    double         gamma;
    double         eps;             /* 1e-8 */
} ppoaf_reward_filter_t;

#define PPOAF_ENV_FILTER_RECORD_LEN(G, W_o, W_c, has_reward) \
    (1 + 2 * (G) * ((W_o) + (W_c) + ((has_reward) ? 1 : 0)))

int ppoaf_env_filter_moments(const ppoaf_obs_filter_t* obs, const ppoaf_obs_filter_t* critic_obs,
                             const ppoaf_reward_filter_t* reward, int32_t G, int64_t n,
                             double* record, ppoaf_stream_t stream);
int ppoaf_env_filter_apply(const ppoaf_obs_filter_t* obs, const ppoaf_obs_filter_t* critic_obs,
                           const ppoaf_reward_filter_t* reward, int32_t G, int64_t n,
                           const double* records /* [R, record_len] */, int32_t R,
                           ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K14  fused ICM mini-batch update
 * replaces one iteration of PPO._icm_batch_train   ppo.py:2487-2567
 *          ICM.forward (encoder x2, inverse model, forward model, both losses)
 *                                                  networks/ppo_networks/icm.py:375-430
 *          LinearObservationEncoder.forward        networks/encoders.py:40-56
 *          mpi_avg_gradients + Adam (no clipping)  ppo.py:2556-2562
 * for the reference's default ICM topology with one width H everywhere:
 *   encoder  O -> H -> H -> H -> H (last layer linear)
 *   inverse  2H -> H (x depth_inv hidden layers) -> A          (softmax + CE for discrete,
 *                                                               MSE for continuous actions)
 *   forward  H + A_in -> H (x depth_fwd hidden layers) -> H     (A_in = classes / action dims)
 * Parameters live in one flat bucket in module order (weight, bias per Linear, each
 * padded to 4 floats): encoder at enc_offset, then inverse, then forward model.
 *
 * `fwd_bwd` enqueues three launches -- encoder forward for both observations (activations
 * to `act_scratch`), inverse / forward model forward + losses + backward (encoding
 * gradients to `denc_scratch`), encoder backward -- each on 2 * ceil(B/16) workgroups of
 * 16 rows, every HxH layer on v_mfma_f32_16x16x4_f32; weight gradients go to per-workgroup
 * slabs.  `reduce` sums the slabs in a fixed order into `grads`, folds the loss into
 * totals[0] (icm_loss = (1-beta) f_loss + beta inv_loss) / totals[1] (count), advances
 * the cursor and, with fused_adam, applies Adam in the same launch (the single-rank path;
 * with more ranks the caller all-reduces `grads` and runs K11).
 * Rows of mini-batch k are perm[k*batch_stride + 0..B) with k read from `cursor`.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t obs_dim, hidden, action_dim, fwd_action_dim, depth_inv, depth_fwd, activation, discrete;
    int64_t enc_offset, inv_offset, fwd_offset, bucket_total;
    const float* params; float* grads; float* exp_avg; float* exp_avg_sq;
    float* slabs;                    /* [2*ceil(B/16), bucket_total]                           */
    int64_t* step_count;             /* [1] Adam step counter (advanced when fused_adam)        */
    const float* lr;                 /* [1] device scalar                                       */
    float beta1, beta2, adam_eps, grad_scale;
    const float* obs;                /* [n_rows, obs_dim]                                       */
    const float* next_obs;           /* [n_rows, obs_dim]                                       */
    const void* actions;             /* int64 [n_rows] (discrete) / float32 [n_rows, action_dim]*/
    const int64_t* perm; const int32_t* row_map; int64_t n_rows;
    int64_t* cursor; int64_t B, batch_stride;
    float icm_beta; int32_t fused_adam;
    float* act_scratch;              /* [2, 4, 16*ceil(B/16), hidden]                           */
    float* denc_scratch;             /* [2, 2, 16*ceil(B/16), hidden]                           */
    float* loss_partials;            /* [ceil(B/16) + 1, 2] (last row: this step's Adam constants)*/
    double* totals;                  /* [2]                                                     */
    /* 1: obs / next_obs / actions are per-epoch tables already in shuffled order (entry i belongs to
     * perm[i]); mini-batch k reads [k * batch_stride, +B) directly, perm / row_map are not consulted */
    int32_t inputs_in_batch_order, _pad;
    /* split-wgrad chain (NULL: every workgroup writes weight-gradient slabs of the bucket).  With a workspace of
     * ppoaf_icm_update_split_workspace_bytes() bytes (256-byte aligned) the three fwd_bwd kernels form NO weight
     * gradient: they publish each layer's dLoss/dz rows (and the inputs the scratch does not hold already), and
     * ppoaf_icm_update_reduce forms every dW = dz^T x once per mini-batch over all rows (both observation streams for the
     * encoder) on f32 MFMA, biases as column sums of dz, [+ Adam on the spot with fused_adam].  Same call sequence and
     * outputs; sums run in MFMA K order (float32-rounding-level differences from the slab form, bitwise reproducible). */
    void* split_workspace; int64_t split_workspace_bytes;
    /* 0: the fwd_bwd launches use every XCD (default).  1 / 2: their workgroups sit on XCDs 0-3 / 4-7 only (the launch is
     * twice as wide and the workgroups dispatched to the other half return at once; workgroup b is dispatched to XCD b % 8):
     * for the PPO update running on the other half at the same time (ppoaf_ppo_update_args_t.xcd_half). */
    int32_t xcd_half;
    /* ABI 6.  1 (with split_workspace, hidden 128; ignored otherwise): ppoaf_icm_update_fwd_bwd issues ONE launch instead of
     * three -- workgroup (tile, stream) runs its stream's encoder, swaps encodings with its partner, runs one of the two
     * models, swaps the encoding gradients and runs its encoder's backward pass; the exchanges are tagged records at the
     * START of split_workspace (ppoaf_icm_update_split_workspace_bytes() includes them), tagged with *cursor + 1: zero the
     * workspace before the first launch and whenever the cursor restarts.  Bitwise the three launches' results.  Word 0 of
     * the workspace is non-zero after a launch in which a partner did not answer within 2 s (results invalid).
     * ppoaf_icm_update_fuses_kernels(args): 1 when these arguments take the single launch. */
    int32_t fuse_kernels;
} ppoaf_icm_update_args_t;

int ppoaf_icm_update_fwd_bwd(const ppoaf_icm_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_icm_update_reduce(const ppoaf_icm_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_icm_update_split_workspace_bytes(const ppoaf_icm_update_args_t* args, int64_t* bytes_out);
int ppoaf_icm_update_fuses_kernels(const ppoaf_icm_update_args_t* args);
/* Rollout-time intrinsic reward of a whole env batch (PPOPolicy.get_intrinsic_reward,
 * policies/ppo_policy.py:954-1007 -> ICM.forward icm.py:375-430 without the inverse model):
 * intr_out[i] = scale * sum_d (forward_model(enc(obs_i), action_i) - enc(next_obs_i))_d^2 with
 * scale = intr_reward_weight * reward_scale / 2.  Uses the same args struct: obs / next_obs /
 * actions hold the B = batch rows directly (perm NULL, fused_adam 0); params, topology and
 * act_scratch as for the update; two launches (encoder for both observations, forward model). */
int ppoaf_icm_intrinsic_reward(const ppoaf_icm_update_args_t* args, float scale, float* intr_out,
                               ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K14, general shapes: the same mini-batch update and rollout-time reward for ICMs whose
 * encoder, encoding and models have widths of their own
 * replaces one iteration of PPO._icm_batch_train   ppo.py:2487-2567
 *          ICM.__init__ / ICM.forward              networks/ppo_networks/icm.py:227-430
 *          LinearObservationEncoder                networks/encoders.py:9-56
 *          PPOPolicy.get_intrinsic_reward          policies/ppo_policy.py:954-1007
 * With pad16(x) = 16 ceil(x / 16):
 *   encoder  O -> E -> E -> E -> D (last layer linear)     E in {32, 64, 128}, 1 <= D <= 128, 1 <= O <= 1024
 *   inverse  2D -> Mi (x depth_inv hidden layers) -> A     Mi, Mf in {32, 64, 128}, depths 1..3, A, A_in <= 8, or <= 16 with n_action_slices, or <= 24 with PPOAF_ICM_WIDE_ACTIONS
 *   forward  D + A_in -> Mf (x depth_fwd hidden layers) -> D
 * Losses, activations and the bucket (module order, each parameter padded to 4 floats) are
 * those of ppoaf_icm_update_args_t.  Weight rows of 2D and D + A_in floats are not 16-byte
 * aligned in general: every layer with a run-time width reads its weights with bound-checked
 * scalar loads; the ExE and MxM layers have compile-time widths.
 *
 * Only the split-wgrad form exists.  `fwd_bwd` enqueues three launches, none of which waits
 * inside a kernel: encoder forward (2 ceil(B/16) workgroups: row tile x obs | next_obs),
 * the two models (row tile x inverse | forward: forward, losses, backward; each model's
 * share of d(enc) to a scratch of its own; ONE launch when inv_hidden == fwd_hidden, else one
 * launch per model), encoder backward (adds the shares as inverse + forward).  `wgrad` is
 * K14's weight-gradient launch over a block table of at most 14 blocks (per-network plane
 * widths; the inverse layer 0 as an enc_1 and an enc_2 block, the forward layer 0 as an enc_1
 * and an action block) [+ Adam with fused_adam], the loss into totals, cursor + 1.  Sums run
 * in a fixed order, no float atomics: bitwise reproducible.
 *   act_scratch   [2][3][Bpad][E] encoder hidden planes, then [2][Bpad][pad16(D)] encodings
 *   denc_scratch  [2 models][2 streams][Bpad][pad16(D)]                 (Bpad = 16 ceil(B/16))
 *   workspace     ppoaf_icm_shapes_workspace_bytes() bytes, 256-byte aligned (update only)
 * `check` validates topology and bucket layout on the host and launches nothing.
 * `intrinsic_reward`: as ppoaf_icm_intrinsic_reward (perm NULL, fused_adam 0; params, topology
 * and act_scratch only), two launches: the encoder, then the forward model alone.
 *
 * Identity encoder (ICM(encoded_obs_dim = 0): obs_encoder = nn.Identity(), icm.py:227-430):
 * enc_hidden == 0 with enc_dim == obs_dim (1 <= O <= 128) and enc_offset == inv_offset (an
 * encoder of size 0; the bucket is the inverse model's parameters, then the forward model's).
 * The encodings are the observation rows: no encoder launch, and no d(enc) -- observations
 * take no gradient.  `fwd_bwd` is the models launch alone (one per model when the widths
 * differ), whose tiles are loaded straight from obs / next_obs (dead rows and columns
 * O .. pad16(O) as zeros); the inverse model's workgroups publish them as the layer-0 panels
 * of `wgrad`, whose table has at most 10 blocks.  `intrinsic_reward` is one launch.
 *   act_scratch   [2][Bpad][pad16(O)]       denc_scratch  unused, may be NULL
 * `check` refuses enc_hidden == 0 with enc_dim != obs_dim or obs_dim > 128.
 *
 * MultiDiscrete actions with equal class counts (n_action_slices = k >= 2): the agent-shared ICM
 * of an agent-grouped policy, one ICM per env over the concatenation of the group's observations
 * with the action space MultiDiscrete([n] * k)          ppo.py:2520-2538, mat_policy.py:1012-1090
 *   discrete = 1, action_dim == fwd_action_dim == k n, n >= 2, k <= 8, action_dim <= 16
 *   actions  int64 [n_rows, k]: slice j of row r at r * k + j (with inputs_in_batch_order the
 *            rows are read as those of the other tables); a class outside [0, n) is clamped into it
 *   forward model input: column j n + a_j of the row's action block is 1 for every slice j -- what
 *            the loop of icm.py:198-211 yields for equal class counts
 *   inverse head: ONE softmax p over the whole action_dim-wide row (icm.py:76-77), then per slice
 *            CrossEntropyLoss on p[slice] (a second log-softmax over the slice), summed over the
 *            slices, mean over B (icm.py:400-412)
 * n_action_slices 0 or 1: Discrete / Box as above, action widths <= 8.  `check` refuses, for
 * k >= 2, discrete == 0, action_dim != fwd_action_dim, k > 8, action_dim > 16, action_dim % k != 0
 * and action_dim / k < 2.
 *
 * Wide actions (opt-in): n_action_slices carries option bits above its low byte, which stays the
 * slice count.  PPOAF_ICM_WIDE_ACTIONS with a slice count of 0 or 1: Discrete / Box with
 * action_dim and fwd_action_dim in [1,24] (discrete needs them equal).  A launch with either
 * above 8 runs the 32-column form of the models and reward kernels (one softmax over the row and
 * CrossEntropyLoss on it, or the MSE over B x A, as at <= 8; the action panels of `wgrad` are
 * [Bpad][32], and the workspace grows by them); with both <= 8 it runs the kernels and needs
 * the workspace it does without the bit.  With a slice count k >= 2 the bit changes nothing:
 * MultiDiscrete keeps k <= 8 and 16 classes.  `check` names the field, its value and [1,24].
 * With the bit, any other bit above the low byte is refused.
 * Without the bit every answer, message and byte count is what it was.
 * ------------------------------------------------------------------------ */
#define PPOAF_ICM_WIDE_ACTIONS 0x100   /* in ppoaf_icm_shapes_args_t.n_action_slices */
typedef struct {
    int32_t obs_dim, enc_hidden, enc_dim, inv_hidden, fwd_hidden, action_dim, fwd_action_dim, depth_inv, depth_fwd;
    int32_t activation, discrete, xcd_half;           /* xcd_half: as ppoaf_icm_update_args_t                */
    int64_t enc_offset, inv_offset, fwd_offset, bucket_total;
    const float* params; float* grads; float* exp_avg; float* exp_avg_sq;
    int64_t* step_count; const float* lr;
    float beta1, beta2, adam_eps, grad_scale;
    const float* obs; const float* next_obs; const void* actions;
    const int64_t* perm; const int32_t* row_map; int64_t n_rows;
    int64_t* cursor; int64_t B, batch_stride;
    float icm_beta; int32_t fused_adam;
    float* act_scratch; float* denc_scratch;
    float* loss_partials;            /* [ceil(B/16) + 1, 2] (last row: this step's Adam constants)*/
    double* totals;                  /* [2]                                                     */
    int32_t inputs_in_batch_order;
    int32_t n_action_slices;         /* 0 | 1: Discrete / Box; k >= 2: MultiDiscrete, k equal slices; | PPOAF_ICM_WIDE_ACTIONS (above) */
    void* workspace; int64_t workspace_bytes;
} ppoaf_icm_shapes_args_t;

int ppoaf_icm_shapes_check(const ppoaf_icm_shapes_args_t* args);
int ppoaf_icm_shapes_workspace_bytes(const ppoaf_icm_shapes_args_t* args, int64_t* bytes_out);
int ppoaf_icm_shapes_fwd_bwd(const ppoaf_icm_shapes_args_t* args, ppoaf_stream_t stream);
int ppoaf_icm_shapes_wgrad(const ppoaf_icm_shapes_args_t* args, ppoaf_stream_t stream);
int ppoaf_icm_shapes_intrinsic_reward(const ppoaf_icm_shapes_args_t* args, float scale, float* intr_out,
                                      ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K15  fused multi-agent-transformer mini-batch update
 * replaces one iteration of PPO._ppo_batch_train for a MATPolicy  ppo.py:2292-2469
 *          MATPolicy.evaluate (token block, teacher forcing)      policies/mat_policy.py:378-439,628-658
 *          MATActorCritic.forward / MATCritic / MATActor          networks/actor_critic/multi_agent_transformer.py:22-373
 *          SelfAttention / Encoding / Decoding blocks             networks/attention.py:13-257
 *          the loss, backward and (through K11) the one clip + Adam over the shared bucket  mat_policy.py:677-699
 * for the default topology: embedding 64, one block, one head, GELU, Discrete actions (<= 8),
 * obs_dim <= 128 (rows up to 32 wide are staged whole in LDS; wider ones stream through it in chunks of
 * 32 columns, read from critic_obs again by the backward), num_agents <= 16.  `offsets` are the 63 parameter tensors of MATActorCritic in
 * module order (each padded to 4 floats) relative to `params`.  Dataset rows are envs carrying
 * num_agents tokens: critic_obs [n_rows, A, O], raw_actions int64 [n_rows, A], advantages /
 * old_log_probs / rewards_to_go / values [n_rows, A].  adv_records / vn_records are (n, mean, M2)
 * float64 per mini-batch over its B*A values ([n_batches, 3] and [n_batches, n_ranks, 3]).
 * `fwd_bwd` = one launch on ceil(B / floor(16/A)) workgroups writing slabs [that many, bucket_total];
 * `reduce` sums them into `grads`, folds the 8 loss scalars + count into totals[9] and advances
 * the cursor; the caller then all-reduces `grads` (N > 1) and runs ppoaf_clip_adam_step.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t obs_dim, num_agents, num_actions, embedding;
    int64_t offsets[64];
    int64_t bucket_total;
    const float* params; float* grads; float* slabs;
    const float* critic_obs; const int64_t* raw_actions;
    const float* advantages; const float* old_log_probs; const float* rewards_to_go; float* values;
    const int64_t* perm; const int32_t* row_map; int64_t n_rows;
    int64_t* cursor; int64_t B, batch_stride;
    int32_t normalize_values, n_ranks, normalize_adv, use_huber;
    float* vn_mean; float* vn_var; double* vn_count;     /* [2] double-buffered by mini-batch parity, as K12 */
    const double* vn_records; const double* adv_records;
    float surr_clip, entropy_weight, kl_loss_weight, huber_delta;
    float* loss_partials;            /* [n_workgroups, 8] */
    double* totals;                  /* [9] */
    /* single-rank fusion of K11's norm pass: with fuse_norm the reduce launch also leaves one partial of ||grads||^2
     * per workgroup -- ppoaf_mat_update_norm_partials(args) of them: ceil(bucket_total / 1024) in the slab form, one per
     * wgrad workgroup with split_workspace -- in norm_scratch[2 ..] (float64[2 + that many], at least
     * PPOAF_NORM_SCRATCH_DOUBLES) and advances step_count, so the caller follows with ppoaf_adam_step_prenormed
     * (n_norm_partials = that count) instead of ppoaf_clip_adam_step */
    double* norm_scratch; int64_t* step_count; int32_t fuse_norm;
    /* 1: critic_obs / raw_actions / advantages / old_log_probs / rewards_to_go are per-epoch tables already in shuffled
     * order (entry i belongs to perm[i]): a mini-batch reads [k * batch_stride, +B) directly, its loads depend on the cursor
     * only; `values` is still written through perm / row_map.  0: they are the rollout buffer's rows. */
    int32_t inputs_in_batch_order;
    /* split-wgrad chain (NULL: every workgroup writes a slab of the whole bucket).  With a workspace of
     * ppoaf_mat_update_split_workspace_bytes() bytes (256-byte aligned) fwd_bwd forms NO weight gradient of the 18
     * 64 x 64 linears -- a third of its MFMA work, all on the one CU that owns a token tile -- and publishes each
     * linear's input and dLoss/dz tile there instead; ppoaf_mat_update_reduce then forms dW = dz^T x once per mini-batch
     * over all tokens (K = every token row, f32 MFMA, one workgroup per 16 x 16 tile), the biases as column sums of dz,
     * and reduces the (now 13 KB) slabs of the small tensors.  Same call sequence, same outputs; sums run in MFMA K order
     * (float32-rounding-level differences from the slab form, bitwise reproducible).  With fuse_norm the launch leaves
     * ppoaf_mat_update_norm_partials(args) partials in norm_scratch[2 ..]. */
    void* split_workspace; int64_t split_workspace_bytes;
    /* mini-batch index = *cursor + mb_offset; the reduce launch adds cursor_advance to *cursor (as K12: eager use (0, 1);
     * a captured chain of n mini-batches bakes mb_offset = 0..n-1 into its nodes and advances the cursor once, by n, in
     * the last one, so all but the first read of the cursor word hit the reader's L2) */
    int64_t mb_offset, cursor_advance;
} ppoaf_mat_update_args_t;

int ppoaf_mat_update_fwd_bwd(const ppoaf_mat_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_mat_update_fwd_bwd_timed(const ppoaf_mat_update_args_t* args, void* start_event, void* stop_event,
                                   ppoaf_stream_t stream);
int ppoaf_mat_update_reduce(const ppoaf_mat_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_mat_update_split_workspace_bytes(const ppoaf_mat_update_args_t* args, int64_t* bytes_out);
/* Fused tail of K15's split-wgrad chain (ABI 5; single rank): ppoaf_mat_update_fwd_bwd -> ppoaf_mat_update_wgrad_adam -- TWO
 * launches per mini-batch.  The weight gradients of the 18 linears and the small tensors (ppoaf_mat_update_reduce's jobs, bit
 * for bit), the clip norm from tagged per-workgroup records every workgroup waits for, and clip + Adam on the workgroup's
 * own elements (mat_policy.py:677-699: one optimiser over actor + critic; ppoaf_adam_step_prenormed's arithmetic) in one
 * launch.  args->fuse_norm must be set (the launch advances step_count); exp_avg / exp_avg_sq / lr / betas / eps / max_norm /
 * grad_norm_out as for ppoaf_adam_step_prenormed.  ctl: ppoaf_mat_update_tail_ctl_bytes() bytes of device memory, 64-byte
 * aligned, zeroed once and kept across launches; its third 32-bit word is non-zero after a launch in which a wait ran out
 * of wait_seconds (results invalid).  All workgroups must be resident together (checked). */
int ppoaf_mat_update_tail_ctl_bytes(const ppoaf_mat_update_args_t* args, int64_t* bytes_out);
int ppoaf_mat_update_wgrad_adam(const ppoaf_mat_update_args_t* args, void* ctl, float* exp_avg, float* exp_avg_sq,
                                const float* lr, float beta1, float beta2, float eps, float grad_scale, float max_norm,
                                float* grad_norm_out, double wait_seconds, ppoaf_stream_t stream);
/* number of squared-norm partials a fuse_norm reduce launch leaves (n_norm_partials of ppoaf_adam_step_prenormed;
 * norm_scratch must hold 2 + that many doubles); -1 on invalid args */
int ppoaf_mat_update_norm_partials(const ppoaf_mat_update_args_t* args);

/* ------------------------------------------------------------------------ *
 * K16  one rollout step of a MATPolicy for all E envs of the rank in one launch
 * replaces MATPolicy.get_rollout_actions / _get_autoregressive_actions  policies/mat_policy.py:441-519,587-626
 *          MATPolicy.get_critic_values + denormalisation               mat_policy.py:660-675, utils/misc.py:124-128
 *          the per-env add_info calls                                   policies/ppo_policy.py:638-651
 * critic_obs: [E, A, obs_dim] (agents of an env side by side, in the policy's slot order); the
 * encoder runs once, the decoder A times (agent i's sampled action is agent i+1's token).
 * Outputs are the step's row of the rollout buffer: actions int64 [E, A], log-probs and
 * (denormalised) values [E, A]; *_copy_out receive the observation rows (actor_obs [E, A,
 * actor_obs_dim], or critic_obs again when NULL).  offsets / limits as K15 (obs_dim <= 128).
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t obs_dim, num_agents, num_actions, embedding, actor_obs_dim, normalize_values;
    int64_t offsets[64];
    const float* params;
    const float* critic_obs; const float* actor_obs; int64_t E;
    uint64_t seed, offset;
    const float* vn_mean; const float* vn_var;
    int64_t* action_out; int64_t* raw_action_out; float* logp_out; float* value_out;
    float* critic_obs_copy_out; float* obs_copy_out;
    const int64_t* forced_action;   /* NULL: sample.  Else [E, A] actions to log instead of sampling (replay) */
} ppoaf_mat_step_args_t;

int ppoaf_mat_policy_step(const ppoaf_mat_step_args_t* args, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K23  the bookkeeping of one env step of a rollout (PPO.rollout), one launch for all of its members
 * replaces, after env.step, per member: the reward / natural-reward rows of its agents,
 *          `reward * ext_reward_weight`, `+ intrinsic reward`, buffer.rewards[t], end_kind[t];
 *          and once: the ep_ts arithmetic of the episode ends                 ppo.py:1795-1983
 * The env's rewards arrive as a ROW-BLOCK TABLE per member, passed by value (no device-side table): block b is the
 * float32 [E] row of the member's b-th agent in env order, wherever it lies -- `base + agent * E` of the env's
 * agent-major tensor, or one tensor of a dict keyed by agent id.  1 <= n_blocks <= PPOAF_ROW_BLOCKS_MAX.
 * Per member, in its buffer layout:
 *   grouped == 0 (PPOPolicy)   row  b * E + e  <- block b, env e                      (agent-major [n * E])
 *   grouped == 1 (MATPolicy)   row  e * n + s  <- block slot_agent[s], env e          ([E, n] in slot order);
 *                              slot_agent is a permutation of 0..n-1 (an entry outside the table is refused)
 *   reward_out[row]  = reward (* ext_reward_weight when it is not 1) (+ intrinsic[row] when intrinsic != NULL):
 *                      two float32 roundings, never one fma -- bitwise the torch statements
 *   natural_out      (NULL: not kept) ALWAYS agent-major, [b * E + e] <- natural[b][e] (reward[b][e] when
 *                      natural[b] == NULL): the layout the rollout statistics sum over
 *   end_kind_out     int8 [n * E] (grouped == 0: the env's kind for each of its agents) or [E] (grouped == 1)
 * write_ends != 0: ts = ep_ts[e] + 1; boot = !terminated[e] && (ts >= max_ts_per_ep || truncated[e] || last_step);
 *   kind = terminated ? 1 : boot ? 2 : 0; ep_ts[e] = (terminated || boot) ? 0 : ts -- ep_ts int32 [E] advances ONCE,
 *   in place; terminated / truncated are byte flags [E] (truncated may be NULL).  write_ends == 0: neither ep_ts nor
 *   end_kind_out is touched (fixed-length rollouts).
 * Alignment: a deliberate exception to the other block tables (ppoaf_policy_step_blocks and
 * ppoaf_mat_policy_step_blocks ask for 16-byte aligned bases).  Here every row is an [E] float32 vector read and written
 * with scalar accesses, and the rows an env hands over lie E * 4 bytes apart (40 bytes at E = 10), so only float32
 * alignment is asked for.  E == 0: PPOAF_OK without a launch.  Plain vector stores; one thread per env.
 * ------------------------------------------------------------------------ */
/* rows of a launch that lie in several tensors are described by a table of this many row-block pointers at most
 * (K23 below, and the block forms of K6+K7 and K16 after it) */
#define PPOAF_ROW_BLOCKS_MAX 16
#define PPOAF_FINISH_MAX_MEMBERS 8
typedef struct {
    int32_t n_blocks, grouped;
    int32_t slot_agent[PPOAF_ROW_BLOCKS_MAX];
    const float* reward[PPOAF_ROW_BLOCKS_MAX];
    const float* natural[PPOAF_ROW_BLOCKS_MAX];
    const float* intrinsic;
    float* reward_out; float* natural_out; int8_t* end_kind_out;
} ppoaf_finish_member_t;

typedef struct {
    int32_t n_members, write_ends, last_step, max_ts_per_ep;
    float ext_reward_weight;
    int64_t E;
    const uint8_t* terminated; const uint8_t* truncated;
    int32_t* ep_ts;
    ppoaf_finish_member_t members[PPOAF_FINISH_MAX_MEMBERS];
} ppoaf_rollout_finish_args_t;

int ppoaf_rollout_finish_rows(const ppoaf_rollout_finish_args_t* args, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K6+K7, block form: ppoaf_policy_step reading the env's tensors where they lie
 * `args` as for ppoaf_policy_step, except that args->obs / args->critic_obs are not read: row r of the launch
 * (0 <= r < args->E = n_blocks * rows_per_block) is row r % rows_per_block of block r / rows_per_block of `obs` and of
 * `critic_obs` -- block a of an agent-major env tensor [A * E, width] is `base + a * E * width`, of a dict env the
 * tensor of the member's a-th agent.  The buffer row (raw actions, actions, log-probs, values, observation copies) is
 * written exactly as by ppoaf_policy_step; the env action of row r ALSO goes to row r % rows_per_block of
 * env_action[r / rows_per_block] (int64 [rows_per_block, 1 or n_action_slices] for the categorical heads, float32
 * [rows_per_block, out_dim] for the Gaussian and Bernoulli ones): the env's combined action tensor or its per-agent
 * tensors, so env.step needs no index_put.  Philox counters, head code and tile code are ppoaf_policy_step's, so for
 * equal inputs, seed and offset every output is bitwise its output on the gathered rows.  A 16-row tile may straddle two
 * blocks: row addresses are computed per row.  Refused: n_blocks outside [1, PPOAF_ROW_BLOCKS_MAX], a base that is null or
 * not 16-byte aligned, args->E != n_blocks * rows_per_block; rows_per_block == 0: PPOAF_OK without a launch.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t n_blocks;
    int64_t rows_per_block;
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
} ppoaf_step_blocks_t;

int ppoaf_policy_step_blocks(const ppoaf_policy_step_args_t* args, const ppoaf_step_blocks_t* blocks, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K16, block form: ppoaf_mat_policy_step reading the env's tensors where they lie
 * `args` as for ppoaf_mat_policy_step, except that args->critic_obs / args->actor_obs are not read.  The table holds one
 * block per agent of the team in env order (n_blocks == args->num_agents), each [E, width] rows; slot s of env e reads
 * row e of block slot_agent[s] of `critic_obs` and of `actor_obs` (all NULL: the actor sees the critic's observation) --
 * K20's slot_agent, but over a table, so a team whose agents are not adjacent in the env works -- on the narrow
 * (obs_dim <= 32) and the wide-chunk path alike.  The buffer row stays grouped [E, A] and is written exactly as by
 * ppoaf_mat_policy_step; the env action of slot s ALSO goes to element e of int64 block env_action[slot_agent[s]].
 * For equal inputs, seed and offset every output is bitwise ppoaf_mat_policy_step's on the regrouped rows.  Refused:
 * n_blocks outside [1, PPOAF_ROW_BLOCKS_MAX] or != num_agents, a base that is null or not 16-byte aligned, a slot_agent
 * entry outside the table or named twice; E == 0: PPOAF_OK without a launch.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t n_blocks;
    int32_t slot_agent[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    const float* actor_obs[PPOAF_ROW_BLOCKS_MAX];
    int64_t* env_action[PPOAF_ROW_BLOCKS_MAX];
} ppoaf_mat_step_blocks_t;

int ppoaf_mat_policy_step_blocks(const ppoaf_mat_step_args_t* args, const ppoaf_mat_step_blocks_t* blocks, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K20  one evaluation step of a MATPolicy for all E envs in one launch
 * replaces MATPolicy.get_inference_actions                              policies/mat_policy.py:701-790
 *          _get_autoregressive_actions_without_exploration (greedy)     mat_policy.py:521-585
 *          _get_autoregressive_actions (sampled)                        mat_policy.py:441-519
 *          (the step of the evaluation loop                             testing.py:8-175)
 * The encoder runs once (up to rep_enc: no value), the decoder A times (agent i's env action is agent i+1's token);
 * only the int64 env actions are stored.  Shapes as K16, but obs_dim <= 64; offsets as K15 (checked).  mode:
 *   PPOAF_INFER_SAMPLE         K16's categorical draw with K16's Philox counter (offset + env * A + slot): for equal
 *                              (obs, params, seed, offset) in grouped layout the actions are bitwise
 *                              ppoaf_mat_policy_step's action_out
 *   PPOAF_INFER_DETERMINISTIC  argmax of the logits, the lowest index on an exact tie; seed / offset are not read
 * Layout: slot s of env e reads the obs_dim floats of observation ROW slot_agent[s] * obs_agent_stride + e * obs_env_stride
 * and writes action ELEMENT slot_agent[s] * act_agent_stride + e * act_env_stride.  slot_agent is the policy's (shuffled)
 * slot order, a permutation of 0..A-1.  Grouped [E, A, .]: env stride A, agent stride 1, identity order; the env's
 * agent-major [A * E, .]: env stride 1, agent stride E, MATPolicy.agent_slot_order().  E == 0: nothing to do.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t obs_dim, num_agents, num_actions, embedding;
    int64_t offsets[64];
    const float* params;
    const float* obs; int64_t E;
    int64_t obs_env_stride, obs_agent_stride;
    int32_t slot_agent[16];
    int32_t mode;
    uint64_t seed, offset;
    int64_t* action_out;
    int64_t act_env_stride, act_agent_stride;
} ppoaf_mat_infer_args_t;

int ppoaf_mat_policy_infer(const ppoaf_mat_infer_args_t* args, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K18  one-layer LSTM network: LSTMNetwork.forward_logits and its gradients
 * replaces nn.LSTM -> LayerNorm -> activation -> ff_layers of
 *          LSTMNetwork.forward                     networks/ppo_networks/lstm.py:103-127
 *          (hidden-state hand-over of the update   ppo.py:2312-2319; its gradients in
 *           ppo.py:2408-2441 via loss.backward)
 * Gate order i, f, g, o (torch's), both b_ih and b_hh; c' = f*c + i*g, h' = o*tanh(c').  The last step's h goes
 * through LayerNorm(hidden) (eps 1e-5, affine) -> activation -> Linear(hidden, ff_hidden) [-> act -> Linear(ff_hidden,
 * ff_hidden)] -> act -> Linear(ff_hidden, out_dim): logits, Gaussian mean or value.  f32 throughout.
 * params / grads point at the network's own bucket: lstm.weight_ih_l0 [4H, in], weight_hh_l0 [4H, H], bias_ih_l0,
 * bias_hh_l0, layer_norm.weight, layer_norm.bias, then weight / bias of each Linear, every tensor padded to 4 floats
 * (module parameter order; anything after them, e.g. a Gaussian log_std, is not touched).
 * x is [rows, steps, in_dim] (batch-first window; steps = 1 for a rollout step), h0 / c0 / hn / cn are [rows, H].
 * Coverage: hidden 32 / 64 / 128, ff_hidden 16 / 32 / 64 / 128, ff_depth 1 / 2, in_dim <= 256, out_dim <= 8,
 * steps <= 16, activation PPOAF_ACT_*.
 * The workspace (floats from ppoaf_lstm_workspace_floats: out[0] = workspace floats, out[1] = bucket floats of the
 * network) holds what the backward passes read; it is sized for rows x steps and written, never cleared, by
 * ppoaf_lstm_forward with stash != 0 (stash == 0: inference, no workspace needed).
 * ppoaf_lstm_backward: d out [rows, out_dim] -> head and LayerNorm gradients and, backwards over the steps, the
 * pre-activation gate gradients of every (row, step) -- into the workspace; no gradient for x, h0, c0 (data).
 * ppoaf_lstm_wgrad: ADDS dW_ih, dW_hh, db (to both b_ih and b_hh), the LayerNorm and Linear gradients to grads;
 * every element is reduced by one workgroup in a fixed order: bitwise reproducible, no atomics.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t in_dim, hidden, ff_hidden, ff_depth, out_dim, activation;
    int64_t rows, steps;
    const float* params;
    float* grads;
    float* workspace;
    int64_t workspace_floats;
} ppoaf_lstm_desc_t;

int ppoaf_lstm_workspace_floats(const ppoaf_lstm_desc_t* desc, int64_t* out /* host [2] */);
int ppoaf_lstm_forward(const ppoaf_lstm_desc_t* desc, const float* x, const float* h0, const float* c0,
                       float* out, float* hn /* NULL ok */, float* cn /* NULL ok */, int32_t stash,
                       ppoaf_stream_t stream);
int ppoaf_lstm_backward(const ppoaf_lstm_desc_t* desc, const float* c0, const float* dout, ppoaf_stream_t stream);
int ppoaf_lstm_wgrad(const ppoaf_lstm_desc_t* desc, const float* x, const float* h0, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K21  one env step of an LSTM actor / critic pair for all E rows in one launch
 * replaces PPOPolicy.get_rollout_actions            policies/ppo_policy.py:729-794
 *          PPO.get_policy_values + denormalisation  ppo.py:1030-1075, utils/misc.py:113-128
 *          the hidden-state rows of add_episode_info policies/ppo_policy.py:593-627
 *          the critic's extra step at a cut         ppo.py:1863-1881
 *          LSTMNetwork.forward                      networks/ppo_networks/lstm.py:103-127
 *          PPOPolicy.get_inference_actions          policies/ppo_policy.py:796-889
 * The networks are K18's (same descriptors, coverage and bucket layout; steps = 1, `rows` is not read: E rules), both
 * with ONE LSTM hidden size (one block size per launch; ff_hidden / ff_depth may differ); the recurrence, LayerNorm
 * and head are K18's forward code at one step, the action heads K6's / K19's (categorical and Gaussian only).
 * obs [E, actor.in_dim], critic_obs [E, critic.in_dim]; actor_h / actor_c / critic_h / critic_c [E, hidden] are the
 * networks' states, stepped IN PLACE.  mode:
 *   PPOAF_LSTM_STEP         2 * ceil(E/16) workgroups (actor / critic halves grouped per XCD as K6's).  Writes row t of
 *                           the rollout buffer as K6 does (raw action, action, log-prob, value -- denormalised when
 *                           normalize_values --, optional observation copies; Philox counter offset + row;
 *                           forced_raw_action as K6's) and the states AFTER the step into the four *_hidden_out /
 *                           *_cell_out rows [E, hidden].
 *   PPOAF_LSTM_CRITIC_NEXT  critic only, ceil(E/16) workgroups: V(critic_obs) (denormalised) -> boot_value_out [E]; the
 *                           critic's (h, c) are replaced only when the device byte *commit != 0.  With `terminated`
 *                           (device bytes [E], 0 / 1) the four stored rows of the terminated envs are zeroed; the
 *                           networks' own state is never reset.
 *   PPOAF_LSTM_INFER        actor only: steps (actor_h, actor_c) and writes the ENVIRONMENT action to action_out in
 *                           K19's layouts ([E] int64 / [E, D] float32); infer_mode = PPOAF_INFER_SAMPLE (K6's draw with
 *                           counter offset + row) or PPOAF_INFER_DETERMINISTIC (argmax, lowest index on a tie /
 *                           tanh(mean) scaled to the bounds).
 *   PPOAF_LSTM_MASK         the zeroing of CRITIC_NEXT alone, for a step without a CRITIC_NEXT launch.
 * ppoaf_lstm_policy_step_check validates the arguments on the host (pointers are only compared with NULL) and
 * launches nothing; E = 0 is accepted by both and launches nothing.
 * ------------------------------------------------------------------------ */
#define PPOAF_LSTM_STEP        0
#define PPOAF_LSTM_CRITIC_NEXT 1
#define PPOAF_LSTM_INFER       2
#define PPOAF_LSTM_MASK        3

typedef struct {
    ppoaf_lstm_desc_t actor, critic;
    const float* obs; const float* critic_obs; int64_t E;
    float* actor_h; float* actor_c; float* critic_h; float* critic_c;
    int32_t head_kind; float min_std;           /* PPOAF_HEAD_CATEGORICAL or PPOAF_HEAD_GAUSSIAN */
    const float* log_std;                       /* Gaussian head: device float32[actor.out_dim] */
    const float* act_lo; const float* act_hi;   /* Gaussian head: bounds per action dimension; both NULL = [-1,1] */
    const void* forced_raw_action;              /* STEP: NULL = sample, else the raw actions to log (as K6) */
    uint64_t seed, offset;
    int32_t normalize_values; int32_t mode;
    const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out; float* value_out;
    float* obs_copy_out; float* critic_obs_copy_out;
    float* actor_hidden_out; float* actor_cell_out; float* critic_hidden_out; float* critic_cell_out;
    int32_t infer_mode; int32_t _pad;
    const uint8_t* commit; const uint8_t* terminated;
    float* boot_value_out;
} ppoaf_lstm_policy_step_args_t;

int ppoaf_lstm_policy_step(const ppoaf_lstm_policy_step_args_t* args, ppoaf_stream_t stream);
int ppoaf_lstm_policy_step_check(const ppoaf_lstm_policy_step_args_t* args);

/* ------------------------------------------------------------------------ *
 * K21, block form: ppoaf_lstm_policy_step reading the env's tensors where they lie
 * `args` as for ppoaf_lstm_policy_step, modes PPOAF_LSTM_STEP and PPOAF_LSTM_CRITIC_NEXT only (MASK reads no observation
 * and INFER runs on gathered rows), except that args->obs / args->critic_obs are not read: row r of the launch
 * (0 <= r < args->E = n_blocks * rows_per_block) is row r % rows_per_block of block r / rows_per_block of `obs` and of
 * `critic_obs` -- block a of an agent-major env tensor [A * E, width] is `base + a * E * width`, of a dict env the
 * tensor of the member's a-th agent.  Everything else stays indexed by the launch row r: the networks' (h, c), the
 * buffer row and the four hidden rows.
 *   STEP         the buffer row (raw actions, actions, log-probs, values, both observation copies, the four hidden rows)
 *                and the stepped (h, c) are written exactly as by ppoaf_lstm_policy_step; the env action of row r ALSO
 *                goes to row r % rows_per_block of env_action[r / rows_per_block] (int64 [rows_per_block] for the
 *                categorical head, float32 [rows_per_block, actor.out_dim] for the Gaussian one): the env's combined
 *                action tensor or its per-agent tensors, so env.step needs no index_put.
 *   CRITIC_NEXT  only `critic_obs` of the table is read (obs / env_action may be NULL); commit and boot_value_out as in
 *                the tensor form.  args->terminated, when given, holds the PER-ENV bytes [rows_per_block] -- the agents
 *                of an env end together -- and row r is zeroed where terminated[r % rows_per_block] is set: the env's
 *                flags are taken as handed, without a copy per agent.
 * Philox counters, head code and tile code are ppoaf_lstm_policy_step's, so for equal inputs, seed and offset every
 * output is bitwise its output on the gathered rows.  A 16-row tile may straddle two blocks (three and more for
 * rows_per_block < 8): row addresses are computed per row.  Loads and stores through the table are scalar, so a base
 * needs its element's alignment only (float32: 4 bytes, int64 actions: 8) -- an env's [E, width] blocks lie
 * E * width * 4 bytes apart, which 16 need not divide.  Refused, before any launch: n_blocks outside
 * [1, PPOAF_ROW_BLOCKS_MAX], args->E != n_blocks * rows_per_block, a base the mode reads or writes that is null or not
 * aligned to its element, a mode other than the two, and whatever ppoaf_lstm_policy_step_check refuses;
 * rows_per_block == 0: PPOAF_OK without a launch.  ppoaf_lstm_policy_step_blocks_check runs the same checks on the host
 * and launches nothing.  Plain vector stores; one lane per row for the heads; no workgroup waits on another.
 * ------------------------------------------------------------------------ */
typedef struct {
    int32_t n_blocks;
    int64_t rows_per_block;
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
} ppoaf_lstm_step_blocks_t;

int ppoaf_lstm_policy_step_blocks(const ppoaf_lstm_policy_step_args_t* args, const ppoaf_lstm_step_blocks_t* blocks,
                                  ppoaf_stream_t stream);
int ppoaf_lstm_policy_step_blocks_check(const ppoaf_lstm_policy_step_args_t* args, const ppoaf_lstm_step_blocks_t* blocks);

/* ------------------------------------------------------------------------ *
 * K22  one mini-batch of the PPO update of an LSTM actor / critic pair as three launches
 * replaces, per mini-batch of PPO._ppo_batch_train    ppo.py:2292-2469
 *          the window gather of the dataset           utils/episode_info.py:775-809,940-987
 *          the hidden-state hand-over and write-back  ppo.py:2312-2319,2450-2466
 *          PPOPolicy.evaluate + the losses            policies/ppo_policy.py:891-952, ppo.py:2325-2438
 *          loss.backward                              ppo.py:2408-2441
 *          clip_grad_norm_ + Adam per network         policies/ppo_policy.py:1037-1042
 * The networks are K18's (same descriptors, coverage and bucket layout; `steps` is the window length S, `rows`,
 * `workspace` and `workspace_floats` of the descriptors are not read), both with ONE LSTM hidden size; actor.params /
 * actor.grads and critic.params / critic.grads point into the policy's flat buckets `params` / `grads` (actor first,
 * critic at actor_size), which also hold a Gaussian head's log_std at log_std_offset floats inside the actor's part.
 * Every launch reads the device cursor: mini-batch mb = *cursor covers entries [mb * batch_stride, mb * batch_stride + B)
 * of `perm` (the epoch's shuffled item indices) and of the per-epoch tables raw_actions / advantages / old_log_probs /
 * rewards_to_go, which hold the items' LAST position (item + S - 1) in shuffled order.
 *   ppoaf_lstm_update_fwd_bwd  2 * ceil(B/16) workgroups (the actor's 16-row tiles, then the critic's) of hidden/16
 *       waves.  A workgroup forms its items' windows -- buffer rows row_map[item + s], s < S, of obs / critic_obs
 *       [n_rows, in_dim]; actor observations zeroed strictly after a terminal position (`terminal`: one byte per
 *       dataset position, NULL when S = 1) --, takes (h0, c0) from the hidden tables [n_rows, hidden] at the last
 *       position's row, stages both into the workspace, runs K18's forward, writes the final (h, c) back to the same
 *       rows, evaluates the head and the loss of its rows (K12's terms; the critic's values are scattered into `values`
 *       at the last position's row; advantage and value normalisation from the per-mini-batch records adv_records
 *       [n_batches, 3] / vn_records [n_batches, n_ranks, 3] of (n, mean, M2) and the double-buffered normaliser slots
 *       vn_mean / vn_var / vn_count [2]), leaves its loss partial sums in loss_partials [2, ceil(B/16), 8] and runs
 *       K18's backward (head, LayerNorm, BPTT) into the workspace.
 *   ppoaf_lstm_update_wgrad    the weight gradients of both networks (K18's tiles: fixed reduction order, no
 *       atomics), STORED into `grads` -- nothing has to clear the bucket --, one pair of squared-norm partials of the
 *       scaled gradient per workgroup in norm_scratch[2 ..]; its last workgroup advances both Adam step counters.
 *   ppoaf_lstm_update_adam     clip norm per network (max_norm <= 0: no clipping) + Adam on exp_avg / exp_avg_sq /
 *       step_counts [2] with the gradient scale grad_scale (1 / ranks); its last workgroup folds loss_partials into the
 *       nine totals, integrates the mini-batch's normaliser record into the other slot and advances the cursor.
 *       norm_mode 0: the partials of ppoaf_lstm_update_wgrad; 1: a norm pass over `grads` first (a fourth launch: after
 *       an all-reduce of the bucket); 2: norm_scratch[0..1] hold the squared norms (ppoaf_peer_exchange_allreduce).
 * ppoaf_lstm_update_check validates on the host only (no launch, no pointer followed; with `pointers` == 0 the shapes
 * alone) and names the offending field; ppoaf_lstm_update_workspace_floats: out[0] = floats of `workspace` for B rows,
 * out[1] = doubles of norm_scratch, out[2] = LDS bytes of a fwd_bwd workgroup.
 * ------------------------------------------------------------------------ */
typedef struct {
    ppoaf_lstm_desc_t actor, critic;
    float* params; float* grads; float* exp_avg; float* exp_avg_sq;
    int64_t bucket_total, actor_size, log_std_offset;     /* log_std_offset: -1 without a Gaussian head */
    int64_t* step_counts; const float* lr; double* norm_scratch; int64_t norm_scratch_doubles;
    float beta1, beta2, adam_eps, grad_scale, max_norm; int32_t head_kind;
    const float* obs; const float* critic_obs; const uint8_t* terminal;
    const int64_t* perm; const int32_t* row_map; int64_t n_rows, n_items;
    const void* raw_actions; const float* advantages; const float* old_log_probs; const float* rewards_to_go;
    float* values;
    float* actor_hidden; float* actor_cell; float* critic_hidden; float* critic_cell;
    int64_t* cursor; int64_t B, batch_stride;
    int32_t normalize_values, n_ranks;
    float* vn_mean; float* vn_var; double* vn_count; const double* vn_records; const double* adv_records;
    int32_t normalize_adv, use_huber;
    float surr_clip, entropy_weight, kl_loss_weight, huber_delta, min_std; int32_t _pad;
    float* loss_partials; double* totals;
    float* workspace; int64_t workspace_floats;
} ppoaf_lstm_update_args_t;

int ppoaf_lstm_update_check(const ppoaf_lstm_update_args_t* args, int32_t pointers);
int ppoaf_lstm_update_workspace_floats(const ppoaf_lstm_update_args_t* args, int64_t* out /* host [3] */);
int ppoaf_lstm_update_fwd_bwd(const ppoaf_lstm_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_lstm_update_wgrad(const ppoaf_lstm_update_args_t* args, ppoaf_stream_t stream);
int ppoaf_lstm_update_adam(const ppoaf_lstm_update_args_t* args, int32_t norm_mode, ppoaf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K17  gradient exchange between the ranks of one node over peer mappings (xGMI)
 * replaces, inside the per-mini-batch update chain, the comm.Allreduce of
 *          mpi_avg_gradients                       utils/mpi_utils.py:65-86  (called from ppo.py:2443-2448,
 *          2557-2558 once per mini-batch; the division by num_procs stays in the optimiser's grad_scale)
 * One process per GPU.  Every rank creates an exchange for its flat gradient bucket, exports an opaque
 * blob (IPC handle of its exchange slots + flag words), the host all-gathers the blobs in rank order over
 * any control plane (torch.distributed, MPI, a file) and every rank connects.  After a host barrier,
 * ppoaf_peer_exchange_allreduce is ONE kernel launch with fixed arguments (hipGraph-capturable):
 *   dst[i] = sum over ranks r = 0..n-1, in that order, of src_r[i]          (bitwise identical on every rank)
 *   norm_out[0] = sum_{i <  split} (norm_scale * dst[i])^2,  norm_out[1] = the same for i >= split
 *                 (double, added in a fixed order; NULL to skip; split_floats >= bucket size: one segment and
 *                 only norm_out[0] is written)
 * dst may alias src.  All ranks must issue the same sequence of exchanges.  A rank waits at most
 * wait_seconds for its peers inside the kernel; on expiry the launch drains, dst is undefined and the error
 * word (status out[1]) holds the sequence number that timed out -- it never hangs.
 * ppoaf_peer_exchange_status: out[0] = exchanges completed, out[1] = 0 or the sequence number of a timed-out
 * wait, out[2] = 1 uncached / 2 fine-grained / 3 coarse-grained exchange memory, out[3] = n_ranks (synchronises the device).
 * ------------------------------------------------------------------------ */
#define PPOAF_PEER_EXCHANGE_MAX_RANKS 16
#define PPOAF_PEER_EXCHANGE_BLOB_BYTES 128
typedef struct ppoaf_peer_exchange ppoaf_peer_exchange_t;

/* memory_kind of the exchange slots: 0 auto (uncached, else fine-grained), 1 uncached, 2 fine-grained, 3 coarse-grained */
int ppoaf_peer_exchange_create(int rank, int n_ranks, int64_t bucket_floats, int memory_kind,
                               ppoaf_peer_exchange_t** out);
int ppoaf_peer_exchange_export(ppoaf_peer_exchange_t* x, void* blob /* host, PPOAF_PEER_EXCHANGE_BLOB_BYTES */);
int ppoaf_peer_exchange_connect(ppoaf_peer_exchange_t* x, const void* all_blobs /* host, n_ranks blobs in rank order */);
int ppoaf_peer_exchange_allreduce(ppoaf_peer_exchange_t* x, const float* src, float* dst, int64_t split_floats,
                                  float norm_scale, double* norm_out, double wait_seconds, ppoaf_stream_t stream);
int ppoaf_peer_exchange_status(ppoaf_peer_exchange_t* x, int64_t* out /* host [4] */);
/* K12 + K17 in one launch: ppoaf_ppo_update_reduce (slabs -> gradient, bookkeeping) whose column sums go from
 * registers into the exchange slot, followed by the cross-rank sum into args->grads; the two clip norms
 * (scaled by args->grad_scale) are left as per-workgroup partials inside the exchange object and are added, in
 * a fixed order, by ppoaf_ppo_update_adam_exchanged -- the Adam launch that must follow on the same stream
 * (ppoaf_ppo_update_adam with the norms taken from the exchange instead of args->norm_scratch).
 * The exchange must have been created for args->bucket_total floats (at most 256 * 1024 of them). */
int ppoaf_ppo_update_reduce_exchange(const ppoaf_ppo_update_args_t* args, ppoaf_peer_exchange_t* x,
                                     double wait_seconds, ppoaf_stream_t stream);
int ppoaf_ppo_update_adam_exchanged(const ppoaf_ppo_update_args_t* args, ppoaf_peer_exchange_t* x,
                                    ppoaf_stream_t stream);
/* The fused tail launch on N > 1 ranks of one node (ABI 5): ppoaf_ppo_update_wgrad_adam with the K17 exchange as a phase
 * of every weight-gradient job (mpi_avg_gradients, utils/mpi_utils.py:89-111, at its call sites ppo_policy.py:1035,1048):
 * workgroup b of every rank forms the same 16 x 32 piece, writes its sums into this rank's slot (16-byte system-scope
 * stores, job-major tiles), flags its peers' group b, reads their tiles back and adds them IN RANK ORDER, then takes part in
 * the launch-wide norm wait and applies clip + Adam (grad_scale = 1 / ranks) to its elements -- two launches per mini-batch,
 * bitwise the same parameters on every rank.  xchg: created for ppoaf_ppo_update_tail_exchange_floats() floats and
 * used by this entry point only (its slot layout is the job list's); not coarse-grained memory (no fences are used);
 * at most 256 workgroups (ppoaf_ppo_update_split_blocks) -- wider shapes use ppoaf_ppo_update_wgrad ->
 * ppoaf_peer_exchange_allreduce -> ppoaf_ppo_update_adam(args, 2, stream).  A peer that does not show up within
 * xchg_wait_seconds sets the exchange's error word (ppoaf_peer_exchange_status) and the launch drains. */
int ppoaf_ppo_update_tail_exchange_floats(const ppoaf_ppo_update_args_t* args, int64_t* floats_out);
int ppoaf_ppo_update_wgrad_adam_exchange(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds,
                                         ppoaf_peer_exchange_t* xchg, double xchg_wait_seconds, ppoaf_stream_t stream);
int ppoaf_peer_exchange_destroy(ppoaf_peer_exchange_t* x);

/* ------------------------------------------------------------------------ *
 * Rank collectives (one communicator per process, one process per GPU; RCCL bound at run time)
 * replaces broadcast_model_parameters   utils/mpi_utils.py:50-63    -> ppoaf_bcast_f32 (flat bucket, once)
 *          mpi_avg / mpi_avg_gradients  utils/mpi_utils.py:65-111   -> ppoaf_allreduce_avg_f32 (sum, then / world)
 *          the raw-data allgather of RunningMeanStd.update  utils/stats.py:47-50
 *                                                                   -> ppoaf_allgather_moments of (n, mean, M2) records
 * Rank 0 creates the id (ppoaf_comm_unique_id), the host distributes its PPOAF_COMM_UNIQUE_ID_BYTES bytes
 * (MPI_Bcast / a file / torch.distributed), every rank calls ppoaf_comm_init (collective).  All calls are
 * asynchronous on `stream` and in place; out of ppoaf_allgather_moments is [world, n_doubles].  They return
 * PPOAF_E_INVALID with a message when no librccl can be bound.  The per-mini-batch gradient exchange inside
 * the update loop has the lower-latency K17 path above; ppo_and_friends_amd's own Python host uses
 * torch.distributed (the same RCCL) for these collectives.
 * ------------------------------------------------------------------------ */
#define PPOAF_COMM_UNIQUE_ID_BYTES 128
typedef struct ppoaf_comm ppoaf_comm_t;

int ppoaf_comm_unique_id(void* out /* host, PPOAF_COMM_UNIQUE_ID_BYTES */);
int ppoaf_comm_init(int rank, int world, const void* unique_id, ppoaf_comm_t** out);
int ppoaf_allreduce_avg_f32(ppoaf_comm_t* comm, float* buf, int64_t n, ppoaf_stream_t stream);
int ppoaf_allreduce_sum_f32(ppoaf_comm_t* comm, float* buf, int64_t n, ppoaf_stream_t stream);   /* sum only */
int ppoaf_bcast_f32(ppoaf_comm_t* comm, float* buf, int64_t n, int root, ppoaf_stream_t stream);
int ppoaf_allgather_moments(ppoaf_comm_t* comm, const double* record, int64_t n_doubles, double* out,
                            ppoaf_stream_t stream);
int ppoaf_comm_destroy(ppoaf_comm_t* comm);
/* mpi_avg_gradients at its per-mini-batch call site (ppo.py:2443-2448) when the K17 peer exchange is not available:
 * fwd_bwd -> reduce -> RCCL sum all-reduce of the gradient bucket -> norms + clip + Adam for n_minibatches consecutive
 * mini-batches (cursor .. cursor + n - 1; the cursor advances by n), all launches issued from this one call (the
 * 1 / world factor is args->grad_scale, as in the three-launch chain).  mb_offset must be 0. */
int ppoaf_ppo_update_chain_allreduce(const ppoaf_ppo_update_args_t* args, ppoaf_comm_t* comm, int64_t n_minibatches,
                                     ppoaf_stream_t stream);
/* The same for the ICM update (ppo.py:2556-2562: averaged gradients, Adam without clipping; args->fused_adam must be 0;
 * norm_scratch as for ppoaf_clip_adam_step) and for the MAT update (mat_policy.py:692-699: one clip + Adam over the
 * shared bucket; args->fuse_norm must be 0, args->norm_scratch / step_count are the optimiser's). */
int ppoaf_icm_update_chain_allreduce(const ppoaf_icm_update_args_t* args, ppoaf_comm_t* comm, int64_t n_minibatches,
                                     double* norm_scratch, float* grad_norm_out /* NULL ok */, ppoaf_stream_t stream);
int ppoaf_mat_update_chain_allreduce(const ppoaf_mat_update_args_t* args, ppoaf_comm_t* comm, int64_t n_minibatches,
                                     float* exp_avg, float* exp_avg_sq, const float* lr /* device [1] */,
                                     float beta1, float beta2, float eps, float grad_scale, float max_norm,
                                     float* grad_norm_out /* NULL ok */, ppoaf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PPOAF_HIP_H */
