// K21 for two stacked LSTM layers: one env step of a two-layer actor / critic pair for every row of a rank in ONE launch.
// Modes, heads, Philox counters, value denormalisation, observation copies, the device byte `commit` and the zeroing of
// terminated envs' stored rows are lstm_policy_step.hip's; what differs is the recurrence.  A state is two rows of H per
// env row: the networks' own [2, E, H] tensors are stepped IN PLACE and the step's rows of the rollout buffer are
// [E, 2, H] -- both are read and written where they lie, through (row stride, layer stride) pairs.
//
// At S = 1 the wavefront of lstm2_forward_kernel has nothing to overlap across time (layer 1 of step 0 needs layer 0 of
// step 0), so the step has a split of its own.  One workgroup per 16-row tile and network, 2 H / 16 waves: waves
// [0, H/16) own layer 0, waves [H/16, 2H/16) layer 1, each wave the hidden slice [16 w, 16 w + 16) of all four gates.
//
//   before barrier 1   every read of the tile's own state rows and of x: h of both layers and x to LDS, c to registers
//   phase A            layer 0: bias0 + x W_ih_l0^T + h0 W_hh_l0^T -> cell -> h0' to LDS
//                      layer 1: h1 W_hh_l1^T from a zero start (the half of its gates that does not wait for layer 0)
//   barrier 2
//   phase B            layer 1: (bias1 + h0' W_ih_l1^T) + phase A's sum -> cell -> h1' to LDS, its (h', c') stored
//                      layer 0: its (h', c') stored in place and into the buffer rows; the observation copy
//   barrier 3          LayerNorm(h1'), activation, feed-forward head on all waves, then the action heads one lane per row
//
// Weights are read once per launch, so nothing is resident: every recurrent fragment streams through one buffer resource
// per matrix (load_fwd_frags_rs), a gate block in flight (half of one at H = 128, as lstm2_forward_kernel reads it).
// The sums are lstm2_forward_kernel's in its order -- (bias + ih) + hh per gate, the H = 128 products in two halves --
// and the cell is lstm2_cell, so the (h', c') a launch leaves are bitwise those of ppoaf_lstm2_forward at S = 1.
//
// LDS map (floats; HS = H + 4):  buf [2 * 16 * kLFS]  x tile (stride kLMaxIn + 4), later the head's two layer buffers
//                                h0o, h1o [16 * HS]   the old h of layer 0 / 1; h0o later the LayerNorm output
//                                h0n, h1n [16 * HS]   the new h of layer 0 / 1
#include <cstddef>

#include "action_heads.hpp"
#include "lstm_stacked_device.hpp"

namespace ppoaf {
namespace {

struct Lstm2StepDev {
    Lstm2Args net[2];                              // actor, critic; h0 / c0 are the states stepped in place
    float* hrow[2]; float* crow[2];                // the step's stored rows of each network (STEP), else null
    long srs, sls;                                 // row and layer stride of the stored rows
    long E;
    int n_wg, mode, head_kind, infer_mode;
    float min_std;
    const float* log_std;
    const float* act_lo; const float* act_hi;
    const void* forced_raw_action;
    unsigned long long seed, offset;
    int normalize_values; const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out;
    float* value_out;                              // values[t] (STEP) or boot_value[t] (CRITIC_NEXT)
    float* obs_out; float* critic_obs_out;
    const unsigned char* commit;                   // CRITIC_NEXT: the critic's states are replaced only when set
    const unsigned char* terminated;
    float* stored[4];                              // the step's hidden rows, for the zeroing
};

// the block form's table, as lstm_policy_step.hip holds it in the kernel arguments
struct Lstm2StepBlocks {
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
    unsigned rows_per_block;
    int action_elems;
};

// where row n of the tile's input lies: dense [E, I], or row n % rows_per_block of block n / rows_per_block
struct XDense2 {
    const float* x;
    __device__ __forceinline__ const float* row(const long n, const int I) const { return x + n * I; }
};
struct XBlocks2 {
    const float* const* blocks;
    unsigned rows_per_block;
    __device__ __forceinline__ const float* row(const long n, const int I) const {
        const unsigned b = (unsigned)n / rows_per_block;
        return blocks[b] + (long)((unsigned)n - b * rows_per_block) * I;
    }
};

// Tile g of network `a`: the two-layer step, LayerNorm and the feed-forward head.  Returns the head's outputs in LDS (row
// stride kLFS), valid for every thread after the call.  `keep`: the stepped states replace the network's own.
template <int H, class XRows>
__device__ __forceinline__ const float* lstm2_rows_step(const Lstm2Args& a, const int g_tile, const XRows xr, float* hrow,
                                                        float* crow, const long srs, const long sls, float* oc,
                                                        const unsigned char* commit) {
    constexpr int HT = H / 16, NW = 2 * HT, NT = NW * 64, HS = H + 4, XS = kLMaxIn + 4;
    static_assert(2 * kLRows * kLFS >= kLRows * XS, "the head's layer buffers reuse the x tile");
    __shared__ __attribute__((aligned(16))) float buf[2 * kLRows * kLFS];
    __shared__ __attribute__((aligned(16))) float h0o[kLRows * HS];
    __shared__ __attribute__((aligned(16))) float h1o[kLRows * HS];
    __shared__ __attribute__((aligned(16))) float h0n[kLRows * HS];
    __shared__ __attribute__((aligned(16))) float h1n[kLRows * HS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the layer branches below are whole-wave branches
    const bool upper = w >= HT;                               // wave-uniform: this wave works on layer 1
    const int wl = upper ? w - HT : w;
    const long r0 = (long)g_tile * kLRows;
    const long N = a.N;
    const int I = a.I, Ip = (a.I + 15) & ~15;
    const int j = 16 * wl + (lane & 15);
    // (both layers' offsets are read and one is picked by arithmetic, as lstm2_forward_kernel does)
    const long up = upper ? 1 : 0;
    const float* Whh = a.P + (a.L.w_hh[0] + up * (a.L.w_hh[1] - a.L.w_hh[0]));
    const long lofs = up * a.ls;
    const __amdgpu_buffer_rsrc_t rsI = frag_rsrc(a.P + a.L.w_ih[1]), rsH = frag_rsrc(Whh), rs0 = frag_rsrc(a.P + a.L.w_ih[0]);
    const unsigned foff = (unsigned)(((16 * wl + (lane & 15)) * H + 4 * (lane >> 4)) * 4);
    const unsigned xoff = (unsigned)((j * I + 4 * (lane >> 4)) * 4);
    auto wih0 = [&](const int disp) __attribute__((always_inline)) {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs0, xoff, disp, 0));
    };
    // init + A (16 rows x H, LDS) x (gate q's rows [16 wl, 16 wl + 16) of the [4H, H] matrix behind rs)^T: the streamed
    // product of lstm2_forward_kernel, chunk for chunk
    constexpr int KC = H == 128 ? HT / 2 : HT;
    auto streamed = [&](const __amdgpu_buffer_rsrc_t rs, const int q, const float* A, const float init) __attribute__((always_inline)) {
        float4 ft[KC];
        if constexpr (KC == HT) {
            __builtin_amdgcn_sched_barrier(0);
            load_fwd_frags_rs<KC>(rs, foff, q * H * H * 4, ft);
            return mfma_rows_x_frags<KC>(A, HS, lane, ft, init);
        } else {
            f32x4 acc = {init, init, init, init};
#pragma unroll
            for (int hh = 0; hh < HT / KC; ++hh) {
                __builtin_amdgcn_sched_barrier(0);            // (one half in flight)
                load_fwd_frags_rs<KC>(rs, foff, (q * H * H + 16 * KC * hh) * 4, ft);
                acc = acc + mfma_rows_x_frags<KC>(A + 16 * KC * hh, HS, lane, ft, 0.f);
            }
            return acc;
        }
    };
    float bias[4];
    {
        const long bi = a.L.b_ih[0] + up * (a.L.b_ih[1] - a.L.b_ih[0]), bh = a.L.b_hh[0] + up * (a.L.b_hh[1] - a.L.b_hh[0]);
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[q] = a.P[bi + q * H + j] + a.P[bh + q * H + j];
    }

    // ---- every read of the tile's own state rows, and of x, before the first barrier: the in-place step is safe
    for (int e = tid; e < kLRows * Ip; e += NT) {
        const int r = e / Ip, k = e - r * Ip;
        const long n = r0 + r;
        buf[r * XS + k] = (n < N && k < I) ? xr.row(n, I)[k] : 0.f;
    }
    for (int e = tid; e < kLRows * H; e += NT) {
        const int r = e / H, k = e - r * H;
        const long n = r0 + r;
        h0o[r * HS + k] = n < N ? a.h0[n * a.rs + k] : 0.f;
        h1o[r * HS + k] = n < N ? a.h0[n * a.rs + a.ls + k] : 0.f;
    }
    float cr[4], hr[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long n = r0 + 4 * (lane >> 4) + g;
        cr[g] = n < N ? a.c0[n * a.rs + lofs + j] : 0.f;
        hr[g] = 0.f;
    }
    const bool keep = commit == nullptr || *commit != 0;
    __syncthreads();

    // ---- phase A
    f32x4 z[4];
    if (!upper) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 acc = {bias[q], bias[q], bias[q], bias[q]};
#pragma unroll 1
            for (int c = 0; c < Ip / 16; ++c) {
                const int k0 = 16 * c + 4 * (lane >> 4);
                const float4 x4 = *reinterpret_cast<const float4*>(buf + (lane & 15) * XS + k0);
                const int wd = (q * H * I + 16 * c) * 4;              // row q H + j of W_ih_l0, columns from 16 c
                const float b0 = k0 < I ? wih0(wd) : 0.f, b1 = k0 + 1 < I ? wih0(wd + 4) : 0.f;
                const float b2 = k0 + 2 < I ? wih0(wd + 8) : 0.f, b3 = k0 + 3 < I ? wih0(wd + 12) : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.x, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.y, b1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.z, b2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.w, b3, acc, 0, 0, 0);
            }
            z[q] = acc + streamed(rsH, q, h0o, 0.f);
        }
        lstm2_cell<H>(a, z, cr, hr, h0n, 0, 0, 0, r0, 0, j, lane);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = streamed(rsH, q, h1o, 0.f);
    }
    __syncthreads();

    // ---- phase B
    if (upper) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 acc = streamed(rsI, q, h0n, bias[q]);
            z[q] = acc + z[q];
        }
        lstm2_cell<H>(a, z, cr, hr, h1n, 0, 0, 0, r0, 0, j, lane);
    } else if (oc) {
        // the observation copy, from the staged tile: layer 0's waves have nothing else to form here
        for (int e = tid; e < kLRows * I; e += NT / 2) {
            const int r = e / I, k = e - r * I;
            if (r0 + r < N) oc[(r0 + r) * I + k] = buf[r * XS + k];
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long n = r0 + 4 * (lane >> 4) + g;
        if (n < N) {
            if (keep) {
                a.hn[n * a.rs + lofs + j] = hr[g];
                a.cn[n * a.rs + lofs + j] = cr[g];
            }
            if (hrow) {
                hrow[n * srs + up * sls + j] = hr[g];
                crow[n * srs + up * sls + j] = cr[g];
            }
        }
    }
    __syncthreads();

    // ---- head: LayerNorm(H) -> activation -> Linear layers on all 2 H / 16 waves; every element's arithmetic is
    //      lstm2_forward_kernel's
    float* A0 = h0o;
    float* A1 = buf;
    float* A2 = buf + kLRows * kLFS;
    for (int r = w; r < kLRows; r += NW) {
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s += h1n[r * HS + k];
        const float mean = wave_sum(s) / (float)H;
        float v = 0.f;
        for (int k = lane; k < H; k += 64) { const float d = h1n[r * HS + k] - mean; v += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(v) / (float)H + 1e-5f);
        for (int k = lane; k < H; k += 64) {
            const float y = (h1n[r * HS + k] - mean) * rstd * a.P[a.L.ln_w + k] + a.P[a.L.ln_b + k];
            A0[r * HS + k] = act_fwd(y, a.act);
        }
    }
    __syncthreads();
    const float* in = A0;
    int IS = HS, K = H;
    for (int l = 0; l <= a.D; ++l) {
        const bool last = l == a.D;
        const int M = last ? a.O : a.F;
        float* ob = (l & 1) ? A2 : A1;
        const float* W = a.P + (l == 0 ? a.L.fw[0] : l == 1 ? a.L.fw[1] : a.L.fw[2]);
        const float* b = a.P + (l == 0 ? a.L.fb[0] : l == 1 ? a.L.fb[1] : a.L.fb[2]);
        for (int e = tid; e < kLRows * M; e += NT) {
            const int r = e / M, m = e - r * M;
            const float* ir = in + r * IS;
            const float* wr = W + (long)m * K;
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += ir[k] * wr[k];
            s += b[m];
            ob[r * kLFS + m] = last ? s : act_fwd(s, a.act);
        }
        __syncthreads();
        in = ob; IS = kLFS; K = M;
    }
    return in;
}

// BLOCKS: the observations are read through the table, STEP also writes the env's action blocks and `terminated` holds
// one byte per row of a block.  Both forms run lstm2_rows_step and the same head functions with the same row number, so
// for equal inputs they store equal bits.
template <int H, bool BLOCKS>
__device__ __forceinline__ void lstm2_step_body(const Lstm2StepDev& u, const Lstm2StepBlocks* tb) {
    constexpr int NT = 2 * (H / 16) * 64;
    const int tid = threadIdx.x;
    int which, g;
    if (u.mode == PPOAF_LSTM_STEP) {
        const int b = blockIdx.x;
        which = (b >> 2) & 1;
        g = ((b >> 3) << 2) | (b & 3);
    } else {
        which = u.mode == PPOAF_LSTM_INFER ? 0 : 1;
        g = blockIdx.x;
    }
    if (g >= u.n_wg) return;
    const long e0 = (long)g * kLRows;

    if (u.mode != PPOAF_LSTM_MASK) {
        const Lstm2Args& a = u.net[which];
        float* oc = which == 0 ? u.obs_out : u.critic_obs_out;
        const unsigned char* commit = which == 1 ? u.commit : nullptr;
        const float* sOut;
        if constexpr (BLOCKS) {
            const XBlocks2 xr{which == 0 ? tb->obs : tb->critic_obs, tb->rows_per_block};
            sOut = lstm2_rows_step<H>(a, g, xr, u.hrow[which], u.crow[which], u.srs, u.sls, oc, commit);
        } else {
            sOut = lstm2_rows_step<H>(a, g, XDense2{a.x}, u.hrow[which], u.crow[which], u.srs, u.sls, oc, commit);
        }

        // heads: one lane per env row
        if (tid < kLRows && e0 + tid < u.E) {
            const float* zr = sOut + tid * kLFS;
            const long e = e0 + tid;
            if (which == 1) {
                float v = zr[0];
                if (u.normalize_values) v = u.vn_mean[0] + v * sqrtf(u.vn_var[0] + 1e-8f);   // misc.py:124-128
                u.value_out[e] = v;
            } else if (u.mode == PPOAF_LSTM_INFER) {
                const bool greedy = u.infer_mode == PPOAF_INFER_DETERMINISTIC;
                if (u.head_kind == PPOAF_HEAD_CATEGORICAL)
                    cat_infer_row(zr, a.O, greedy, e, u.seed, u.offset, u.action_out);
                else
                    gauss_infer_row(zr, a.O, greedy, u.log_std, u.min_std, u.act_lo, u.act_hi, e, u.seed, u.offset,
                                    u.action_out);
            } else if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
                cat_step_row(zr, a.O, u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out, u.action_out, u.logp_out);
                if constexpr (BLOCKS) {
                    const unsigned b = (unsigned)e / tb->rows_per_block;
                    const long r = (long)((unsigned)e - b * tb->rows_per_block);
                    reinterpret_cast<int64_t*>(tb->env_action[b])[r] = reinterpret_cast<const int64_t*>(u.action_out)[e];
                }
            } else {
                gauss_step_row(zr, a.O, u.log_std, u.min_std, u.act_lo, u.act_hi, u.forced_raw_action, e, u.seed, u.offset,
                               u.raw_action_out, u.action_out, u.logp_out);
                if constexpr (BLOCKS) {
                    const unsigned b = (unsigned)e / tb->rows_per_block;
                    const long r = (long)((unsigned)e - b * tb->rows_per_block);
                    const int n = tb->action_elems;
                    const float* src = reinterpret_cast<const float*>(u.action_out) + e * n;
                    float* dst = reinterpret_cast<float*>(tb->env_action[b]) + r * n;
                    for (int k = 0; k < n; ++k) dst[k] = src[k];
                }
            }
        }
    }

    // the rows the step stored for the envs that terminated at it: both layers zeroed in all four tensors (the networks'
    // own state is not reset)
    if (u.terminated && (u.mode == PPOAF_LSTM_CRITIC_NEXT || u.mode == PPOAF_LSTM_MASK)) {
        for (int i = tid; i < kLRows * 2 * H; i += NT) {
            const int r = i / (2 * H), k = i - r * 2 * H;
            const long n = e0 + r;
            bool dead = false;
            if (n < u.E) {
                if constexpr (BLOCKS) dead = u.terminated[(unsigned)n % tb->rows_per_block] != 0;
                else dead = u.terminated[n] != 0;
            }
            if (dead) {
                const long at = n * u.srs + (k >= H ? u.sls + (k - H) : k);
#pragma unroll
                for (int q = 0; q < 4; ++q) u.stored[q][at] = 0.f;
            }
        }
    }
}

template <int H>
__global__ __launch_bounds__(2 * (H / 16) * 64) PPOAF_NO_PK_F32 void lstm2_policy_step_kernel(const Lstm2StepDev u) {
    lstm2_step_body<H, false>(u, nullptr);
}

template <int H>
__global__ __launch_bounds__(2 * (H / 16) * 64) PPOAF_NO_PK_F32 void lstm2_policy_step_blocks_kernel(const Lstm2StepDev u,
                                                                                                    const Lstm2StepBlocks tb) {
    lstm2_step_body<H, true>(u, &tb);
}

template <int H>
int launch_step(const Lstm2StepDev& u, const Lstm2StepBlocks* tb, hipStream_t s) {
    const unsigned grid = u.mode == PPOAF_LSTM_STEP ? 8u * (unsigned)((u.n_wg + 3) / 4) : (unsigned)u.n_wg;
    const dim3 block(2 * (H / 16) * 64);
    if (tb) {
        hipLaunchKernelGGL(lstm2_policy_step_blocks_kernel<H>, dim3(grid), block, 0, s, u, *tb);
        return check_launch("lstm2_policy_step_blocks");
    }
    hipLaunchKernelGGL(lstm2_policy_step_kernel<H>, dim3(grid), block, 0, s, u);
    return check_launch("lstm2_policy_step");
}

// a network's descriptor as the launch reads it: E rows of one step (the descriptor's own `rows` is not read)
int check_step_desc(const ppoaf_lstm2_desc_t* d, const long E, const char* what) {
    ppoaf_lstm2_desc_t one = *d;
    one.rows = E > 0 ? E : 1;
    if (E == 0) { one.state_row_stride = one.hidden; one.state_layer_stride = one.hidden; }     // no row: no stride is used
    return check_lstm2_desc(&one, false, what);
}

// with_obs: obs / critic_obs are read from `a` (the block form reads them through its table)
int check_step_args(const ppoaf_lstm2_policy_step_args_t* a, const bool with_obs = true) {
    PPOAF_REQUIRE(a, "lstm2_policy_step: null args");
    PPOAF_REQUIRE(a->mode >= PPOAF_LSTM_STEP && a->mode <= PPOAF_LSTM_MASK,
                  "lstm2_policy_step: mode=%d (0 step, 1 critic next, 2 infer, 3 mask)", a->mode);
    PPOAF_REQUIRE(a->E >= 0, "lstm2_policy_step: negative E");
    PPOAF_REQUIRE(a->E <= (1L << 27), "lstm2_policy_step: E too large");
    if (int rc = check_step_desc(&a->actor, a->E, "lstm2_policy_step: actor")) return rc;
    if (int rc = check_step_desc(&a->critic, a->E, "lstm2_policy_step: critic")) return rc;
    PPOAF_REQUIRE(a->actor.hidden == a->critic.hidden,
                  "lstm2_policy_step: LSTM hidden sizes differ (actor %d, critic %d): one launch has one block size",
                  a->actor.hidden, a->critic.hidden);
    PPOAF_REQUIRE(a->actor.steps == 1 && a->critic.steps == 1, "lstm2_policy_step: steps must be 1");
    PPOAF_REQUIRE(a->critic.out_dim == 1, "lstm2_policy_step: critic out_dim must be 1");
    PPOAF_REQUIRE(a->head_kind == PPOAF_HEAD_CATEGORICAL || a->head_kind == PPOAF_HEAD_GAUSSIAN,
                  "lstm2_policy_step: head_kind=%d (0 categorical, 1 Gaussian)", a->head_kind);
    PPOAF_REQUIRE(a->head_kind != PPOAF_HEAD_GAUSSIAN || a->log_std, "lstm2_policy_step: the Gaussian head needs log_std");
    PPOAF_REQUIRE((a->act_lo == nullptr) == (a->act_hi == nullptr), "lstm2_policy_step: give both action bounds or neither");
    const bool rows = a->actor_hidden_out && a->actor_cell_out && a->critic_hidden_out && a->critic_cell_out;
    if (rows || a->mode == PPOAF_LSTM_STEP || a->mode == PPOAF_LSTM_MASK) {
        const long H = a->actor.hidden, rs = a->stored_row_stride, ls = a->stored_layer_stride;
        PPOAF_REQUIRE((rs == 2 * H && ls == H) || (rs == H && ls == a->E * H),
                      "lstm2_policy_step: stored strides (row %ld, layer %ld) describe neither [E, 2, %ld] nor [2, E, %ld]", rs, ls, H,
                      H);
    }
    if (a->mode == PPOAF_LSTM_STEP) {
        PPOAF_REQUIRE((!with_obs || (a->obs && a->critic_obs)) && a->actor_h && a->actor_c && a->critic_h && a->critic_c,
                      "lstm2_policy_step: STEP: null observation / state pointer");
        PPOAF_REQUIRE(a->raw_action_out && a->action_out && a->logp_out && a->value_out && rows,
                      "lstm2_policy_step: STEP needs the row-t outputs (actions, log-probs, values, four hidden rows)");
    } else if (a->mode == PPOAF_LSTM_CRITIC_NEXT) {
        PPOAF_REQUIRE((!with_obs || a->critic_obs) && a->critic_h && a->critic_c && a->boot_value_out && a->commit,
                      "lstm2_policy_step: CRITIC_NEXT: null critic_obs / critic state / boot_value_out / commit");
        PPOAF_REQUIRE(!a->terminated || rows, "lstm2_policy_step: terminated given without the four hidden rows");
    } else if (a->mode == PPOAF_LSTM_INFER) {
        PPOAF_REQUIRE(a->obs && a->actor_h && a->actor_c && a->action_out,
                      "lstm2_policy_step: INFER: null obs / actor state / action_out");
        PPOAF_REQUIRE(a->infer_mode == PPOAF_INFER_SAMPLE || a->infer_mode == PPOAF_INFER_DETERMINISTIC,
                      "lstm2_policy_step: infer_mode=%d (0 sample, 1 deterministic)", a->infer_mode);
    } else {
        PPOAF_REQUIRE(a->terminated && rows, "lstm2_policy_step: MASK needs terminated and the four hidden rows");
    }
    if (a->mode == PPOAF_LSTM_STEP || a->mode == PPOAF_LSTM_CRITIC_NEXT)
        PPOAF_REQUIRE(!a->normalize_values || (a->vn_mean && a->vn_var), "lstm2_policy_step: normaliser state missing");
    return PPOAF_OK;
}

int check_step_blocks(const ppoaf_lstm2_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t) {
    PPOAF_REQUIRE(a && t, "lstm2_policy_step_blocks: null args");
    PPOAF_REQUIRE(a->mode == PPOAF_LSTM_STEP || a->mode == PPOAF_LSTM_CRITIC_NEXT,
                  "lstm2_policy_step_blocks: mode=%d (0 step, 1 critic next; INFER and MASK have no block form)", a->mode);
    PPOAF_REQUIRE(t->n_blocks >= 1 && t->n_blocks <= PPOAF_ROW_BLOCKS_MAX, "lstm2_policy_step_blocks: n_blocks=%d not in [1, %d]",
                  t->n_blocks, PPOAF_ROW_BLOCKS_MAX);
    PPOAF_REQUIRE(t->rows_per_block >= 0, "lstm2_policy_step_blocks: rows_per_block=%ld must be >= 0", (long)t->rows_per_block);
    PPOAF_REQUIRE(a->E == t->rows_per_block * t->n_blocks,
                  "lstm2_policy_step_blocks: E=%ld is not n_blocks=%d x rows_per_block=%ld", (long)a->E, t->n_blocks,
                  (long)t->rows_per_block);
    // scalar loads and stores: the element's own alignment is all that is asked for
    const uintptr_t act_mask = a->head_kind == PPOAF_HEAD_GAUSSIAN ? 3 : 7;
    for (int b = 0; b < t->n_blocks; ++b) {
        PPOAF_REQUIRE(t->critic_obs[b] && ((uintptr_t)t->critic_obs[b] & 3) == 0,
                      "lstm2_policy_step_blocks: block %d: the critic_obs base is null or not aligned to 4 bytes", b);
        if (a->mode == PPOAF_LSTM_STEP)
            PPOAF_REQUIRE(t->obs[b] && t->env_action[b] && ((uintptr_t)t->obs[b] & 3) == 0 &&
                              ((uintptr_t)t->env_action[b] & act_mask) == 0,
                          "lstm2_policy_step_blocks: block %d: the obs / env_action base is null or not aligned to its element "
                          "(float32 4 bytes, int64 8)", b);
    }
    return check_step_args(a, false);
}

// the device view of checked arguments
Lstm2StepDev step_dev_of(const ppoaf_lstm2_policy_step_args_t* a) {
    Lstm2StepDev u{};
    for (int w = 0; w < 2; ++w) {
        ppoaf_lstm2_desc_t d = w == 0 ? a->actor : a->critic;
        d.rows = a->E; d.steps = 1;
        u.net[w] = lstm2_args_of(&d);
        u.net[w].ws = nullptr; u.net[w].stash = 0;
    }
    Lstm2Args& ac = u.net[0];
    Lstm2Args& cr = u.net[1];
    ac.x = a->obs; ac.h0 = ac.hn = a->actor_h; ac.c0 = ac.cn = a->actor_c;
    cr.x = a->critic_obs; cr.h0 = cr.hn = a->critic_h; cr.c0 = cr.cn = a->critic_c;
    u.value_out = a->value_out;
    u.srs = a->stored_row_stride; u.sls = a->stored_layer_stride;
    if (a->mode == PPOAF_LSTM_STEP) {
        u.hrow[0] = a->actor_hidden_out; u.crow[0] = a->actor_cell_out;
        u.hrow[1] = a->critic_hidden_out; u.crow[1] = a->critic_cell_out;
        u.obs_out = a->obs_copy_out; u.critic_obs_out = a->critic_obs_copy_out;
    } else if (a->mode == PPOAF_LSTM_CRITIC_NEXT) {
        u.commit = a->commit;
        u.value_out = a->boot_value_out;
    }
    u.E = a->E;
    u.n_wg = (int)((a->E + kLRows - 1) / kLRows);
    u.mode = a->mode; u.head_kind = a->head_kind; u.infer_mode = a->infer_mode; u.min_std = a->min_std;
    u.log_std = a->log_std; u.act_lo = a->act_lo; u.act_hi = a->act_hi;
    u.forced_raw_action = a->mode == PPOAF_LSTM_STEP ? a->forced_raw_action : nullptr;
    u.seed = a->seed; u.offset = a->offset;
    u.normalize_values = a->normalize_values; u.vn_mean = a->vn_mean; u.vn_var = a->vn_var;
    u.raw_action_out = a->raw_action_out; u.action_out = a->action_out; u.logp_out = a->logp_out;
    u.terminated = (a->mode == PPOAF_LSTM_CRITIC_NEXT || a->mode == PPOAF_LSTM_MASK) ? a->terminated : nullptr;
    u.stored[0] = a->actor_hidden_out; u.stored[1] = a->actor_cell_out;
    u.stored[2] = a->critic_hidden_out; u.stored[3] = a->critic_cell_out;
    return u;
}

int launch_for(const int H, const Lstm2StepDev& u, const Lstm2StepBlocks* tb, hipStream_t s) {
    switch (H) {
        case 32: return launch_step<32>(u, tb, s);
        case 64: return launch_step<64>(u, tb, s);
    }
    return launch_step<128>(u, tb, s);
}

}  // namespace
}  // namespace ppoaf

using namespace ppoaf;

// the layout the ctypes structure of _lib.py restates (tests/test_lstm_layers_step_scope.py reads this list)
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, actor, 0);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic, 88);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, obs, 176);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_obs, 184);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, E, 192);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, actor_h, 200);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, actor_c, 208);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_h, 216);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_c, 224);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, head_kind, 232);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, min_std, 236);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, log_std, 240);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, act_lo, 248);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, act_hi, 256);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, forced_raw_action, 264);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, seed, 272);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, offset, 280);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, normalize_values, 288);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, mode, 292);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, vn_mean, 296);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, vn_var, 304);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, raw_action_out, 312);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, action_out, 320);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, logp_out, 328);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, value_out, 336);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, obs_copy_out, 344);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_obs_copy_out, 352);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, actor_hidden_out, 360);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, actor_cell_out, 368);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_hidden_out, 376);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, critic_cell_out, 384);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, infer_mode, 392);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, _pad, 396);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, commit, 400);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, terminated, 408);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, boot_value_out, 416);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, stored_row_stride, 424);
PPOAF_LAYOUT(ppoaf_lstm2_policy_step_args_t, stored_layer_stride, 432);
static_assert(sizeof(ppoaf_lstm2_policy_step_args_t) == 440, "ppoaf_lstm2_policy_step_args_t");

extern "C" int ppoaf_lstm2_policy_step_check(const ppoaf_lstm2_policy_step_args_t* a) { return check_step_args(a); }

extern "C" int ppoaf_lstm2_policy_step(const ppoaf_lstm2_policy_step_args_t* a, ppoaf_stream_t stream) {
    if (int rc = check_step_args(a)) return rc;
    if (a->E == 0) return PPOAF_OK;
    return launch_for(a->actor.hidden, step_dev_of(a), nullptr, (hipStream_t)stream);
}

extern "C" int ppoaf_lstm2_policy_step_blocks_check(const ppoaf_lstm2_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t) {
    return check_step_blocks(a, t);
}

extern "C" int ppoaf_lstm2_policy_step_blocks(const ppoaf_lstm2_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t,
                                              ppoaf_stream_t stream) {
    if (int rc = check_step_blocks(a, t)) return rc;
    if (a->E == 0) return PPOAF_OK;                 // no row: nothing is read, nothing launched
    Lstm2StepDev u = step_dev_of(a);
    u.net[0].x = u.net[1].x = nullptr;
    Lstm2StepBlocks tb;
    for (int b = 0; b < PPOAF_ROW_BLOCKS_MAX; ++b) {
        const bool in = b < t->n_blocks;
        tb.obs[b] = in && a->mode == PPOAF_LSTM_STEP ? t->obs[b] : nullptr;
        tb.critic_obs[b] = in ? t->critic_obs[b] : nullptr;
        tb.env_action[b] = in && a->mode == PPOAF_LSTM_STEP ? t->env_action[b] : nullptr;
    }
    tb.rows_per_block = (unsigned)t->rows_per_block;
    tb.action_elems = a->head_kind == PPOAF_HEAD_GAUSSIAN ? a->actor.out_dim : 1;
    return launch_for(a->actor.hidden, u, &tb, (hipStream_t)stream);
}
