// Box (tanh-Gaussian) form of the MAT kernels K15, K16 and K20 (mat_update.hip): what differs from the Discrete form.
//   MATActor with continuous actions (networks/actor_critic/multi_agent_transformer.py:22-156): the action encoder is
//   Linear(NA, 64) WITH a bias over the previous agents' actions themselves (no start-token column: slot 0 sees zeros,
//   mat_policy.py:308-344), the head's last linear gives the means of a GaussianDistribution (networks/distributions.py:
//   441-694) whose log_std is a parameter of the bucket.
// Everything between the encoder and the head is the Discrete kernels' code (mat_device.hpp): the pieces here are called from
// `if constexpr (BOX)` branches of the same kernel bodies.
//   K15: the token block of evaluate (mat_policy.py:378-439: slot i sees the STORED raw action of slot i - 1) and the
//        token's own raw action [16][8] (the 512 bytes behind the 34 activation tiles); the head on wave 0, four lanes per
//        token row, lane (row, q) owning dimensions q and q + 4 -- two transcendental chains per lane instead of eight,
//        row sums by quad permutes, as the Discrete head beside it.  The log_std gradient of the workgroup's 16 rows is
//        folded over the row lanes (xor shuffles over lane bits 2 .. 5) and stored as the workgroup's partial in its
//        compact slab; the wgrad launch adds the partials in slab order with the other small tensors.
//   K16: one lane per token row draws with K6's gauss_step_row (action_heads.hpp): the row's Philox counter is
//        offset + env * A + slot, block q of it gives the normals of dimensions 4 q .. 4 q + 3; the REFINED action is
//        agent i + 1's token (mat_policy.py:441-519).
//   K20: a lane pair per token row, lane (row, q) drawing and refining dimensions 4 q .. 4 q + 3 from Philox block q
//        (mat_box_infer_lane); only the refined env actions leave the kernel (mat_policy.py:521-585,701-790).
#pragma once
#include "action_heads.hpp"

namespace ppoaf {

// K15: stored raw actions -> the action-token tile (row s + 1 of a sequence <- the action of row s) and the rows' own
// actions.  tok_of(s): index of token row s in `actions` ([tokens][NA]).  n_rows * NA <= 128: one pass.
template <class TokOf>
__device__ __forceinline__ void mat_box_action_tiles(const float* __restrict__ actions, const TokOf tok_of,
                                                     const int* __restrict__ sRow, const int n_rows, const int L, const int NA,
                                                     const int xs, float* __restrict__ sXA, float* __restrict__ sRaw,
                                                     const int tid) {
    if (tid < n_rows * NA) {
        const int s = tid / NA, d = tid - s * NA;
        if (sRow[s] >= 0) {
            const float v = actions[tok_of(s) * NA + d];
            sRaw[s * 8 + d] = v;
            if (s % L + 1 < L) sXA[(s + 1) * xs + d] = v;
        }
    }
}

// K15, wave 0: tanh-Gaussian log-prob / entropy of the 16 token rows, the PPO surrogate, d loss / d mean -> sDOutA, the
// workgroup's log_std-gradient partial -> slab_ls[pad4(NA)], the tile's loss partials -> lp[8] (the Discrete head's slots)
__device__ __forceinline__ void mat_box_head_wave0(const float* __restrict__ sOutA, const float* __restrict__ sRaw,
                                                   const float* __restrict__ log_std, const float min_std, const int NA,
                                                   const bool live4, const float av4, const float lpo4, const float surr_clip,
                                                   const float entropy_weight, const float inv_n,
                                                   float* __restrict__ sDOutA, float* __restrict__ slab_ls,
                                                   float* __restrict__ lp, const float adv_mean, const float adv_std,
                                                   const int lane) {
    const int s4 = lane >> 2, q = lane & 3;
    const int k0 = q, k1 = q + 4;
    const bool v0 = k0 < NA, v1 = k1 < NA;
    float mu0 = 0.f, x0 = 0.f, ls0 = 0.f, mu1 = 0.f, x1 = 0.f, ls1 = 0.f;
    float l = 0.f, slog = 0.f, ent = 0.f;
    if (v0) {
        mu0 = sOutA[s4 * 8 + k0]; x0 = live4 ? sRaw[s4 * 8 + k0] : 0.f; ls0 = log_std[k0];
        gauss_dim_terms(mu0, x0, ls0, min_std, l, slog, ent);
    }
    if (v1) {
        mu1 = sOutA[s4 * 8 + k1]; x1 = live4 ? sRaw[s4 * 8 + k1] : 0.f; ls1 = log_std[k1];
        gauss_dim_terms(mu1, x1, ls1, min_std, l, slog, ent);
    }
    const float logp4 = group4_sum(l) - group4_sum(slog);
    const float ent4 = group4_sum(ent);
    const float ratio = expf(logp4 - lpo4);
    const float bad4 = (isnan(ratio) || isinf(ratio)) ? 1.f : 0.f;
    const float lo = 1.0f - surr_clip, hi = 1.0f + surr_clip;
    const float surr1 = ratio * av4, surr2 = fminf(fmaxf(ratio, lo), hi) * av4;
    float glp;
    if (surr1 <= surr2) glp = -av4 * ratio;
    else glp = (ratio >= lo && ratio <= hi) ? -av4 * ratio : 0.f;
    glp *= inv_n;
    const float gH = (entropy_weight != 0.0f) ? -entropy_weight * inv_n : 0.f;
    float dm0 = 0.f, dl0 = 0.f, dm1 = 0.f, dl1 = 0.f;
    if (v0) gauss_dim_grads(mu0, x0, ls0, min_std, glp, gH, dm0, dl0);
    if (v1) gauss_dim_grads(mu1, x1, ls1, min_std, glp, gH, dm1, dl1);
    sDOutA[s4 * 8 + k0] = (live4 && v0) ? dm0 : 0.f;
    sDOutA[s4 * 8 + k1] = (live4 && v1) ? dm1 : 0.f;
    // log_std: this workgroup's rows, dimension by dimension (lanes of equal q differ in bits 2 .. 5)
    float t0 = (live4 && v0) ? dl0 : 0.f, t1 = (live4 && v1) ? dl1 : 0.f;
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) { t0 += __shfl_xor(t0, m, 64); t1 += __shfl_xor(t1, m, 64); }
    if (lane < 4) {
        slab_ls[k0] = t0;
        if (k1 < ((NA + 3) & ~3)) slab_ls[k1] = t1;
    }
    // row results -> lane s (= row s) for the partial sums of the tile
    const int src = (lane & 15) * 4;
    const float r_live = __shfl(live4 ? 1.f : 0.f, src, 64);
    const float r_surr = __shfl(-fminf(surr1, surr2), src, 64), r_ent = __shfl(ent4, src, 64);
    const float r_kl = __shfl(lpo4 - logp4, src, 64), r_bad = __shfl(bad4, src, 64);
    const bool row_live = lane < kRows && r_live != 0.f;
    const float p0 = group16_sum(row_live ? r_surr : 0.f), p3 = group16_sum(row_live ? r_ent : 0.f);
    const float p4 = group16_sum(row_live ? r_kl : 0.f), p7 = group16_sum(row_live ? r_bad : 0.f);
    if (lane == 0) {
        lp[0] = p0; lp[1] = 0.f; lp[3] = p3; lp[4] = p4; lp[7] = p7;
        lp[5] = adv_mean; lp[6] = adv_std;
    }
}

// K16, pass i: the lane of token row `tok` samples (or, with `forced`, evaluates the recorded raw action), logs raw
// action, refined action and log-prob, and hands the refined action on: next_token (NULL for the last agent) is the
// row of agent i + 1 in the LDS action tile, env_row (NULL outside the block form) the env's own action row
__device__ __forceinline__ void mat_box_step_row(const float* __restrict__ mean_row, const int NA,
                                                 const float* __restrict__ log_std, const float min_std,
                                                 const float* __restrict__ act_lo, const float* __restrict__ act_hi,
                                                 const float* __restrict__ forced, const long tok,
                                                 const unsigned long long seed, const unsigned long long offset,
                                                 float* raw_out, float* action_out, float* __restrict__ logp_out,
                                                 float* __restrict__ next_token, float* __restrict__ env_row) {
    gauss_step_row(mean_row, NA, log_std, min_std, act_lo, act_hi, forced, tok, seed, offset, raw_out, action_out, logp_out);
    for (int d = 0; d < NA; ++d) {
        const float a = action_out[tok * NA + d];
        if (next_token) next_token[d] = a;
        if (env_row) env_row[d] = a;
    }
}

// K20, pass i: a LANE PAIR per token row.  Lane (row, q) owns dimensions 4 q .. 4 q + 3 -- exactly Philox block q of the
// row's counter `ctr` (= offset + env * A + slot, K16's), so with NA <= 8 a row is two lanes with one Box-Muller block
// each, side by side.  The per-dimension arithmetic is gauss_step_row's, operation for operation (the sampled actions
// are bitwise K16's action_out); greedy: tanh(mean) scaled to the bounds, the counter is not read.  The refined action
// goes to the env's row and, with next_token (NULL for the last agent), into agent i + 1's row of the LDS action tile --
// before the barrier that pass i + 1's decoder reads behind.  No log-prob, no raw action.
__device__ __forceinline__ void mat_box_infer_lane(const float* __restrict__ mean_row, const int NA, const int q,
                                                   const bool greedy, const float* __restrict__ log_std, const float min_std,
                                                   const float* __restrict__ act_lo, const float* __restrict__ act_hi,
                                                   const unsigned long long seed, const unsigned long long ctr,
                                                   float* __restrict__ env_row, float* __restrict__ next_token) {
    const bool rescale = act_lo != nullptr;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!greedy) gauss_normals4(seed, ctr, (uint32_t)q, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = 4 * q + j;
        if (d < NA) {
            const float mean = mean_row[d];
            float x = mean;
            if (!greedy) {
                const float sd = fmaxf(softplus_u(log_std[d]), min_std);
                x = mean + sd * z[j];
            }
            float a = tanhf(x);
            if (rescale) a = unit_to_bounds(a, act_lo[d], act_hi[d]);
            env_row[d] = a;
            if (next_token) next_token[d] = a;
        }
    }
}

}  // namespace ppoaf
