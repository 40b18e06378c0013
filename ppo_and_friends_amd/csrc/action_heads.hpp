// Action heads on <= 8 actor outputs (Categorical and tanh-Gaussian: <= 24 for the wide heads of the 256/512 pair), one lane
// per row.  The Categorical and tanh-Gaussian rows of a rollout step and of
// an evaluation step: one copy for the MLP kernels (K6, K19) and the LSTM kernel (K21).  The MultiDiscrete and
// MultiBinary heads: shared by the rollout step (K6+K7,
// policy_step.hip) and the fused update (K12, ppo_update_dev.hpp: ppo_head_loss).  Both take a row's log-prob from the
// same functions here, on output values formed by the same output-layer code, so the log-prob logged for a row and the
// one its first mini-batch recomputes are bitwise equal.
//   MultiDiscrete(nvec)  networks/distributions.py:272-438, output function :1047-1064: slice j = outputs
//                        [o_j, o_j + nvec[j]); per slice softmax -> Categorical(probs) (renormalised, clamp_probs, log);
//                        log-prob and entropy are sums over the slices.
//   MultiBinary(n)       :134-196, output function :1111-1113: torch Bernoulli(probs = sigmoid(z)), whose logits are
//                        l = log q - log1p(-q), q = clamp(p, eps, 1 - eps); log-prob = -BCEWithLogits(l, a), entropy =
//                        BCEWithLogits(l, p) with the unclamped p as the target, both summed over the bits.
// Per-class values live in float[8] register arrays that are only ever indexed by unrolled loop counters (a runtime index
// would put them in scratch); slices are walked through a bit mask instead.
#pragma once
#include "mlp_device.hpp"

namespace ppoaf {

// ---- host: the head fields of ppoaf_ppo_update_args_t / ppoaf_policy_step_args_t
inline int check_action_head(const char* what, int head_kind, const ppoaf_mlp_desc_t& actor, int n_slices,
                             const int32_t* slices) {
    PPOAF_REQUIRE(head_kind >= PPOAF_HEAD_CATEGORICAL && head_kind <= PPOAF_HEAD_BERNOULLI,
                  "%s: head_kind=%d (0 categorical, 1 Gaussian, 2 multi-categorical, 3 Bernoulli)", what, head_kind);
    if (head_kind == PPOAF_HEAD_GAUSSIAN) {
        PPOAF_REQUIRE(actor.log_std_offset >= 0, "%s: log_std offset must be given exactly for the Gaussian head", what);
        return PPOAF_OK;
    }
    PPOAF_REQUIRE(actor.log_std_offset < 0, "%s: log_std offset must be given exactly for the Gaussian head (head_kind=%d)",
                  what, head_kind);
    if (head_kind == PPOAF_HEAD_MULTI_CATEGORICAL) {
        PPOAF_REQUIRE(n_slices >= 1 && n_slices <= 8, "%s: n_action_slices=%d out of [1,8]", what, n_slices);
        int sum = 0;
        for (int j = 0; j < n_slices; ++j) {
            PPOAF_REQUIRE(slices[j] >= 1, "%s: action_slices[%d]=%d (every slice needs >= 1 class)", what, j, slices[j]);
            sum += slices[j];
        }
        PPOAF_REQUIRE(sum == actor.out_dim, "%s: action_slices sum to %d, the actor has %d outputs", what, sum,
                      actor.out_dim);
    }
    return PPOAF_OK;       // (Bernoulli: one bit per actor output; out_dim <= 8 is checked with the network)
}

// ---- sampling pieces shared by the rollout step (K6) and the evaluation step (K19, policy_infer.hip): one copy, so
// that a sampled evaluation action is bitwise the rollout's for the same (outputs, seed, counter)
// Discrete: softmax of the row's <= K outputs -> p (padding classes 0); returns the sum of p (Categorical's own
// renormaliser, ~1).  K = 8, or 24 for the wide heads of the 256/512 pair (instantiations of their own): classes 0 .. 7 take
// the same operations in the same order under both.
template <int K = 8>
__device__ __forceinline__ float cat_probs(const float* z, const int out_dim, float* p) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) if (k < out_dim) m = fmaxf(m, z[k]);
    float ssum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = k < out_dim ? expf(z[k] - m) : 0.f; ssum += p[k]; }
    const float inv = 1.0f / ssum;
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] *= inv; s2 += p[k]; }
    return s2;
}
// the row with Philox counter `ctr` draws (seed, ctr, 0).x and takes the inverse CDF over the unnormalised mass
template <int K = 8>
__device__ __forceinline__ int cat_sample(const float* p, const float s2, const int out_dim,
                                          const unsigned long long seed, const unsigned long long ctr) {
    int a = out_dim - 1;
    float c = 0.f;
    const Philox4 rnd = philox4x32_10(seed, ctr, 0u);
    const float uu = u32_to_unit(rnd.x) * s2;
    bool found = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k < out_dim) {
            c += p[k];
            if (!found && uu < c) { a = k; found = true; }
        }
    }
    return a;
}
// Box: four standard normals (Box-Muller on the Philox block (seed, ctr, q)) for action dimensions 4 q .. 4 q + 3
__device__ __forceinline__ void gauss_normals4(const unsigned long long seed, const unsigned long long ctr,
                                               const uint32_t q, float* z) {
    const Philox4 r = philox4x32_10(seed, ctr, q);
    const float u0 = u32_to_unit_open0(r.x), u1 = u32_to_unit(r.y);
    const float u2 = u32_to_unit_open0(r.z), u3 = u32_to_unit(r.w);
    const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
    float sa, ca, sb, cb;
    sincosf(6.28318530717958647692f * u1, &sa, &ca);
    sincosf(6.28318530717958647692f * u3, &sb, &cb);
    z[0] = ra * ca; z[1] = ra * sa; z[2] = rb * cb; z[3] = rb * sb;
}
// a squashed action in [-1, 1] -> [lo, hi]                                          distributions.py:580-581
__device__ __forceinline__ float unit_to_bounds(float a, float lo, float hi) { return ((a + 1.0f) / 2.0f) * (hi - lo) + lo; }
// ---- one row of the Categorical / tanh-Gaussian head, one lane per row: the rollout step (K6, policy_step.hip, and K21,
// lstm_policy_step.hip, share the *_step_row pair) and the evaluation step (K19, policy_infer.hip, and K21's INFER mode
// share the *_infer_row pair).  z / mean: the row's outputs; the row's Philox counter is offset + e.
// Discrete: sample (or the forced raw action, clamped into the classes) -> raw action, action, log-prob
template <int K = 8>
__device__ __forceinline__ void cat_step_row(const float* z, const int out_dim, const void* forced_raw_action, const long e,
                                             const unsigned long long seed, const unsigned long long offset,
                                             void* raw_action_out, void* action_out, float* logp_out) {
    float p[K];
    const float s2 = cat_probs<K>(z, out_dim, p);
    int a;
    float pa = p[0];
    if (forced_raw_action) {
        const long fa = reinterpret_cast<const int64_t*>(forced_raw_action)[e];
        a = fa < 0 ? 0 : (fa >= out_dim ? out_dim - 1 : (int)fa);
    } else {
        a = cat_sample<K>(p, s2, out_dim, seed, offset + (unsigned long long)e);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) if (k == a) pa = p[k];
    reinterpret_cast<int64_t*>(raw_action_out)[e] = a;
    reinterpret_cast<int64_t*>(action_out)[e] = a;
    logp_out[e] = logf(clamp_prob_u(pa / s2));
}
// Box: x = mean + sd * normal (or the forced raw action) -> raw action, tanh(x) scaled to the bounds (act_lo NULL: the
// unit box), log-prob of the squashed Gaussian
__device__ __forceinline__ void gauss_step_row(const float* mean_row, const int out_dim, const float* log_std,
                                               const float min_std, const float* act_lo, const float* act_hi,
                                               const void* forced_raw_action, const long e, const unsigned long long seed,
                                               const unsigned long long offset, void* raw_action_out, void* action_out,
                                               float* logp_out) {
    float* raw = reinterpret_cast<float*>(raw_action_out) + e * out_dim;
    float* ac = reinterpret_cast<float*>(action_out) + e * out_dim;
    const bool rescale = act_lo != nullptr;
    const float* forced = reinterpret_cast<const float*>(forced_raw_action);
    float lp = 0.f, slog = 0.f;
    for (int d0 = 0; d0 < out_dim; d0 += 4) {
        float z[4];
        gauss_normals4(seed, offset + (unsigned long long)e, (uint32_t)(d0 >> 2), z);
        for (int j = 0; j < 4 && d0 + j < out_dim; ++j) {
            const int d = d0 + j;
            const float sd = fmaxf(softplus_u(log_std[d]), min_std);
            const float mean = mean_row[d];
            const float x = forced ? forced[e * out_dim + d] : mean + sd * z[j];
            raw[d] = x;
            float a = tanhf(x);
            slog += logf(fmaxf(1.0f - a * a, 1e-6f));
            if (rescale) a = unit_to_bounds(a, act_lo[d], act_hi[d]);
            ac[d] = a;
            const float zz = x - mean;
            float l = -(zz * zz) / (2.0f * sd * sd) - logf(sd) - 0.91893853320467274178f;
            lp += fminf(fmaxf(l, -100.f), 100.f);
        }
    }
    logp_out[e] = lp - slog;
}
// Discrete, evaluation: the argmax, the lowest index on an exact tie (torch.argmax on the reference's CPU tensors), or a
// sample -> the env action
template <int K = 8>
__device__ __forceinline__ void cat_infer_row(const float* zr, const int out_dim, const bool greedy, const long e,
                                              const unsigned long long seed, const unsigned long long offset,
                                              void* action_out) {
    int a = 0;
    if (greedy) {
        float best = zr[0];
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (k < out_dim && zr[k] > best) { best = zr[k]; a = k; }
    } else {
        float p[K];
        const float s2 = cat_probs<K>(zr, out_dim, p);
        a = cat_sample<K>(p, s2, out_dim, seed, offset + (unsigned long long)e);
    }
    reinterpret_cast<int64_t*>(action_out)[e] = a;
}
// Box, evaluation: tanh(mean), or tanh of a sample, scaled to the bounds -> the env action
__device__ __forceinline__ void gauss_infer_row(const float* zr, const int out_dim, const bool greedy, const float* log_std,
                                                const float min_std, const float* act_lo, const float* act_hi, const long e,
                                                const unsigned long long seed, const unsigned long long offset,
                                                void* action_out) {
    float* ac = reinterpret_cast<float*>(action_out) + e * out_dim;
    const bool rescale = act_lo != nullptr;
    for (int d0 = 0; d0 < out_dim; d0 += 4) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (!greedy) gauss_normals4(seed, offset + (unsigned long long)e, (uint32_t)(d0 >> 2), z);
        for (int j = 0; j < 4 && d0 + j < out_dim; ++j) {
            const int d = d0 + j;
            const float mean = zr[d];
            float x = mean;
            if (!greedy) {
                const float sd = fmaxf(softplus_u(log_std[d]), min_std);
                x = mean + sd * z[j];
            }
            float a = tanhf(x);
            if (rescale) a = unit_to_bounds(a, act_lo[d], act_hi[d]);
            ac[d] = a;
        }
    }
}
// MultiBinary: the uniform of bit d = component d % 4 of Philox (seed, ctr, d / 4); r carries the block from bit to bit
__device__ __forceinline__ float bern_uniform(const unsigned long long seed, const unsigned long long ctr, const int d,
                                              Philox4& r) {
    if ((d & 3) == 0) r = philox4x32_10(seed, ctr, (uint32_t)(d >> 2));
    const uint32_t w = (d & 3) == 0 ? r.x : ((d & 3) == 1 ? r.y : ((d & 3) == 2 ? r.z : r.w));
    return u32_to_unit(w);
}

// ---- MultiDiscrete
// bit k set where class k opens a slice; every class from sum(nvec) on opens one of its own, so no slice runs into padding
__device__ __forceinline__ unsigned mcat_starts(const int n_slices, const int* nvec) {
    unsigned first = 0u;
    int o = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < n_slices) { first |= 1u << o; o += nvec[j]; }
    return first | (0xffu << o);
}

// every class <- the max / the sum of its slice, formed in ascending class order (as distributions.hip's softmax_row)
template <bool MAX>
__device__ __forceinline__ void slice_totals(const float* v, float* t, const unsigned first) {
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        r = ((first >> k) & 1u) ? v[k] : (MAX ? fmaxf(r, v[k]) : r + v[k]);
        t[k] = r;
    }
#pragma unroll
    for (int k = 6; k >= 0; --k)
        if (!((first >> (k + 1)) & 1u)) t[k] = t[k + 1];
}

// per-slice F.softmax -> p; the slice's sum of p (Categorical's own renormaliser, ~1) -> s.  Padding classes: p = 0.
__device__ __forceinline__ void mcat_probs(const float* z, const unsigned first, const int out_dim, float* p, float* s) {
    float t[8];
    slice_totals<true>(z, t, first);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = k < out_dim ? expf(z[k] - t[k]) : 0.f;
    slice_totals<false>(p, t, first);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = k < out_dim ? p[k] * (1.0f / t[k]) : 0.f;
    slice_totals<false>(p, s, first);
}

// the chosen class of every slice as a mask, bit o_j + a_j (a_j clamped into the slice, as the categorical head does)
template <typename I>
__device__ __forceinline__ unsigned mcat_pick(const I* a, const int n_slices, const int* nvec) {
    unsigned pick = 0u;
    int o = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < n_slices) {
            const long c = (long)a[j];
            pick |= 1u << (o + (c < 0 ? 0 : (c >= nvec[j] ? nvec[j] - 1 : (int)c)));
            o += nvec[j];
        }
    }
    return pick;
}

// K6: slice j of env row e draws Philox (seed, offset + j * E + e, 0).x and takes the inverse CDF over the unnormalised
// mass (distributions.hip: categorical_sample_kernel) -- the counters of the torch path's per-slice samples
__device__ __forceinline__ unsigned mcat_sample(const float* p, const float* s, const unsigned first, const int out_dim,
                                                const unsigned long long seed, const unsigned long long offset,
                                                const long E, const long e) {
    unsigned pick = 0u;
    int j = -1;
    float uu = 0.f, c = 0.f;
    bool found = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < out_dim) {
            if ((first >> k) & 1u) {
                ++j;
                const Philox4 r = philox4x32_10(seed, offset + (unsigned long long)j * E + e, 0u);
                uu = u32_to_unit(r.x) * s[k];
                c = 0.f;
                found = false;
            }
            c += p[k];
            if (!found && (uu < c || ((first >> (k + 1)) & 1u))) { pick |= 1u << k; found = true; }
        }
    }
    return pick;
}

// log-prob of the chosen classes: the slices' log(clamp(p / s)), summed in slice order
__device__ __forceinline__ float mcat_logp(const float* p, const float* s, const unsigned pick) {
    float lp = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((pick >> k) & 1u) lp += logf(clamp_prob_u(p[k] / s[k]));
    return lp;
}

// K12: the sum of the slice entropies, and d loss / d z -> dz for d loss / d log-prob = glp, d loss / d entropy = gH:
// the categorical head's chain z -softmax-> p -(/sum)-> n -clamp,log-> l, slice by slice
__device__ __forceinline__ float mcat_entropy_grad(const float* p, const float* s, const unsigned first,
                                                   const unsigned pick, const int out_dim, const float glp,
                                                   const float gH, float* dz) {
    float g[8], h[8], t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        g[k] = 0.f; h[k] = 0.f; t[k] = 0.f;
        if (k < out_dim) {
            const float nk = p[k] / s[k], ck = clamp_prob_u(nk), lk = logf(ck);
            const float in_range = (nk >= FLT_EPSILON && nk <= 1.0f - FLT_EPSILON) ? 1.f : 0.f;
            h[k] = -(nk * lk);
            float gk = gH * (-lk - nk * in_range / ck);
            if ((pick >> k) & 1u) gk += glp * in_range / ck;
            g[k] = gk;
            t[k] = gk * nk;
        }
    }
    slice_totals<false>(h, h, first);
    float ent = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < out_dim && ((first >> k) & 1u)) ent += h[k];
    slice_totals<false>(t, t, first);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        g[k] = k < out_dim ? (g[k] - t[k]) / s[k] : 0.f;
        h[k] = g[k] * p[k];
    }
    slice_totals<false>(h, t, first);
#pragma unroll
    for (int k = 0; k < 8; ++k) dz[k] = k < out_dim ? p[k] * (g[k] - t[k]) : 0.f;
    return ent;
}

// ---- MultiBinary
__device__ __forceinline__ float sigmoid_u(float x) { return 1.0f / (1.0f + expf(-x)); }
// torch's probs_to_logits(is_binary=True) of the clamped probability q
__device__ __forceinline__ float bern_logit(float q) { return logf(q) - log1pf(-q); }
// BCEWithLogits(l, t) = (1 - t) l - log sigmoid(l)
__device__ __forceinline__ float bce_with_logits(float l, float t) {
    return (1.0f - t) * l - (fminf(l, 0.f) - log1pf(expf(-fabsf(l))));
}

// log-prob of the bits a[0 .. n)
template <typename A>
__device__ __forceinline__ float bern_logp(const float* z, const A& a, const int n) {
    float lp = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if (d < n) lp -= bce_with_logits(bern_logit(clamp_prob_u(sigmoid_u(z[d]))), a[d]);
    return lp;
}

// K12: entropy, and d loss / d z -> dz as torch autograd forms it: the clamp passes no gradient outside [eps, 1 - eps]
// (bounds included); the entropy's target p carries a term of its own everywhere
template <typename A>
__device__ __forceinline__ float bern_entropy_grad(const float* z, const A& a, const int n, const float glp,
                                                   const float gH, float* dz) {
    float ent = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        dz[d] = 0.f;
        if (d < n) {
            const float p = sigmoid_u(z[d]), q = clamp_prob_u(p), l = bern_logit(q);
            ent += bce_with_logits(l, p);
            const float sl = sigmoid_u(l);
            const float in_range = (p >= FLT_EPSILON && p <= 1.0f - FLT_EPSILON) ? 1.f : 0.f;
            const float gl = glp * (a[d] - sl) + gH * (sl - p);                 // d / dl of -BCE(l, a) and of BCE(l, p)
            const float gp = gl * in_range * (1.0f / q + 1.0f / (1.0f - q)) - gH * l;
            dz[d] = gp * (1.0f - p) * p;
        }
    }
    return ent;
}

}  // namespace ppoaf
