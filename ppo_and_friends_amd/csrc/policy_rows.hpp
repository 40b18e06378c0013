// The device views of the rollout step (K6+K7, policy_step.hip) and of the evaluation step (K19, policy_infer.hip) and the
// rollout step's 16-row body, shared with the translation unit that holds the kernels of the wide heads of the 256/512 pair
// (policy_wide_heads.hip: 9 .. 24 actor outputs, Categorical and tanh-Gaussian).
#pragma once
#include <cstddef>
#include "ppo_update_dev.hpp"        // the list of instantiated width pairs (and action_heads.hpp)

namespace ppoaf {

constexpr int kThreadsS = kThreadsU;

struct StepDev {
    NetDev net[2];
    const float* params;
    const float* obs; const float* critic_obs; long E;
    int head_kind; float min_std;
    const float* act_lo; const float* act_hi;      // per action dimension, NULL: [-1, 1] (no rescale)
    const void* forced_raw_action;                 // NULL: sample; else the raw actions to log (replay / teacher forcing)
    unsigned long long seed, offset;
    int normalize_values; const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out; float* value_out;
    float* obs_out; float* critic_obs_out;     // buffer rows for the observation copies (may be NULL)
    int n_wg;
    int n_slices; int slices[8];               // multi-categorical head: classes per action dimension
};

// The block form (ppoaf_policy_step_blocks): row r of the launch is row r % rows_per_block of block r / rows_per_block
// of `obs` / `critic_obs`, and its env action also goes to that row of `env_action`.  The pointers travel in the kernel
// arguments.
struct StepBlocks {
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
    long rows_per_block;
    int action_elems, action_is_float;         // elements of one row's env action; float32 (Box, MultiBinary) or int64
};

extern __shared__ __attribute__((aligned(16))) unsigned char policy_step_smem[];

// XH: the MultiDiscrete / MultiBinary heads are compiled in (instantiations of their own, so that the categorical and
// Gaussian ones keep their registers)
// KO: the actor outputs the carve and the Categorical row hold, 8 or kWideOut (the wide heads: never with XH)
template <int HT, bool XH, bool BLK = false, int KO = 8>
__device__ __forceinline__ void policy_step_body(const StepDev& u, const int which, const int g,
                                                 const StepBlocks* tb = nullptr) {
    static_assert(KO == 8 || !XH, "the wide heads are Categorical and tanh-Gaussian");
    constexpr int OS = mlp_rows_out_stride(KO);
    const int tid = threadIdx.x;
    const NetDev& nd = u.net[which];
    const int out_dim = nd.out_dim;
    const float* P = u.params + nd.offset;
    const long e0 = (long)g * kRows;
    // the forward K19 runs as well (mlp_device.hpp)
    float* smem = reinterpret_cast<float*>(policy_step_smem);
    float* cpy = which == 0 ? u.obs_out : u.critic_obs_out;
    const float* sOut;
    if constexpr (BLK) {
        const BlockRows rows{which == 0 ? tb->obs : tb->critic_obs, tb->rows_per_block};
        sOut = mlp_rows_forward<HT, BlockRows, KO>(nd, u.params, nullptr, cpy, u.E, e0, smem, &rows);
    } else {
        sOut = mlp_rows_forward<HT, void, KO>(nd, u.params, which == 0 ? u.obs : u.critic_obs, cpy, u.E, e0, smem);
    }

    // heads: one lane per env row
    if (tid < kRows && e0 + tid < u.E) {
        const int s = tid;
        const long e = e0 + s;
        if (which == 1) {
            float v = sOut[s * OS];
            if (u.normalize_values) v = u.vn_mean[0] + v * sqrtf(u.vn_var[0] + 1e-8f);   // misc.py:124-128
            u.value_out[e] = v;
        } else if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
            cat_step_row<KO>(sOut + s * OS, out_dim, u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out,
                             u.action_out, u.logp_out);
        } else if (XH) {
            // MultiDiscrete / MultiBinary: the log-prob by the functions K12 recomputes it with (action_heads.hpp)
            float z[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) z[k] = k < out_dim ? sOut[s * OS + k] : 0.f;
            if (u.head_kind == PPOAF_HEAD_MULTI_CATEGORICAL) {
                const int D = u.n_slices;
                const unsigned first = mcat_starts(D, u.slices);
                float p[8], sm[8];
                mcat_probs(z, first, out_dim, p, sm);
                const unsigned pick = u.forced_raw_action
                    ? mcat_pick(reinterpret_cast<const int64_t*>(u.forced_raw_action) + e * D, D, u.slices)
                    : mcat_sample(p, sm, first, out_dim, u.seed, u.offset, u.E, e);
                int64_t* raw = reinterpret_cast<int64_t*>(u.raw_action_out) + e * D;
                int64_t* ac = reinterpret_cast<int64_t*>(u.action_out) + e * D;
                int j = -1, o = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k < out_dim) {
                        if ((first >> k) & 1u) { ++j; o = k; }
                        if ((pick >> k) & 1u) { raw[j] = k - o; ac[j] = k - o; }
                    }
                }
                u.logp_out[e] = mcat_logp(p, sm, pick);
            } else {
                // bit d = u_d < sigmoid(z_d), u_d = component d % 4 of Philox (seed, offset + e, d / 4)
                const float* forced = reinterpret_cast<const float*>(u.forced_raw_action);
                float* raw = reinterpret_cast<float*>(u.raw_action_out) + e * out_dim;
                float* ac = reinterpret_cast<float*>(u.action_out) + e * out_dim;
                float a[8];
                Philox4 r = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    a[d] = 0.f;
                    if (d < out_dim) {
                        if (forced) {
                            a[d] = forced[e * out_dim + d];
                        } else {
                            a[d] = bern_uniform(u.seed, u.offset + (unsigned long long)e, d, r) < sigmoid_u(z[d]) ? 1.f : 0.f;
                        }
                        raw[d] = a[d];
                        ac[d] = a[d];
                    }
                }
                u.logp_out[e] = bern_logp(z, a, out_dim);
            }
        } else {
            gauss_step_row(sOut + s * OS, out_dim, P + nd.log_std_off, u.min_std, u.act_lo, u.act_hi,
                           u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out, u.action_out, u.logp_out);
        }
        if (BLK && which == 0) {
            // the row's env action, as this lane has just stored it in the buffer row, into the env's action tensor
            const long b = e / tb->rows_per_block, r = e - b * tb->rows_per_block;
            const int n = tb->action_elems;
            if (tb->action_is_float) {
                const float* src = reinterpret_cast<const float*>(u.action_out) + e * n;
                float* dst = reinterpret_cast<float*>(tb->env_action[b]) + r * n;
                for (int k = 0; k < n; ++k) dst[k] = src[k];
            } else {
                const int64_t* src = reinterpret_cast<const int64_t*>(u.action_out) + e * n;
                int64_t* dst = reinterpret_cast<int64_t*>(tb->env_action[b]) + r * n;
                for (int k = 0; k < n; ++k) dst[k] = src[k];
            }
        }
    }
}

// the launches of the wide heads (policy_wide_heads.hip): net[0].out_dim in 9 .. kWideOut at a wide pair, Categorical or Gaussian
int launch_step_wide_heads(const StepDev& u, size_t lds, hipStream_t s);
int launch_step_blocks_wide_heads(const StepDev& u, const StepBlocks& tb, size_t lds, hipStream_t s);

// ---- K19
struct InferDev {
    NetDev net;
    const float* params;
    const float* obs; long E;
    int head_kind, mode; float min_std;
    const float* act_lo; const float* act_hi;
    unsigned long long seed, offset;
    void* action_out;
    int n_slices; int slices[8];
};

extern __shared__ __attribute__((aligned(16))) unsigned char policy_infer_smem[];

// the launch of the wide heads (policy_wide_heads.hip): a 256-wide actor with 9 .. kWideOut outputs, Categorical or Gaussian
int launch_infer_wide_heads(const InferDev& u, size_t lds, hipStream_t s);

}  // namespace ppoaf
