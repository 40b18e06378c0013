// K14 for general shapes (see include/ppoaf_hip.h: ppoaf_icm_shapes_args_t): the ICM mini-batch update and the
// rollout-time intrinsic reward for an encoder O -> E -> E -> E -> D and models of widths Mi / Mf, each of its own.
//   icm_sh_encoder_fwd_kernel<E/16>   obs / next_obs rows -> hidden planes, encodings [2][Bpad][pad16(D)]
//   icm_sh_models_kernel<M/16>        inverse | forward model: forward, loss, backward; d(enc) shares to scratch
//   icm_sh_encoder_bwd_kernel<E/16>   d(enc) = inverse's share + forward's share -> dgrad through the encoder
//   icm_wgrad_kernel (icm_update.hip) every dW = dz^T x over a block table with per-network plane widths [+ Adam]
// Split-wgrad form only: no slabs, no workgroup pairs, nothing waits inside a kernel.  Work decomposition as K14's:
// 16 rows per workgroup, wave w owns output columns [16 w, +16), activations in LDS, f32 MFMA.  The ExE / MxM layers
// have compile-time widths (mlp_device.hpp: layer_fwd / layer_dgrad); every layer with D, 2D, D + A_in or O on one side
// has run-time sizes and reads its weights with bound-checked scalar loads (rows of 18 or 12 floats at the baseline
// shapes are not 16-byte aligned), as the encoder's layer 0 (K = O) always has.  Columns D .. pad16(D) of every
// D-wide panel are written as zeros.
// MultiDiscrete actions (n_action_slices = k >= 2, the agent-shared ICM of a MAT group): A = A_in = k n <= 16, `actions`
// int64 [rows][k]; the forward model's input carries k one-hots side by side, the inverse head takes one softmax over
// the row and a cross entropy per slice (icm.py:76-77, 198-211, 400-412) in icm_sh_models_kernel<., 16>.
// Identity encoder (enc_hidden = 0, D = O <= 128): the encodings ARE the observation rows.  No encoder kernel runs; the
// models kernel and the reward kernel fill their two encoding tiles from the observation tables (sh_load_obs), the
// inverse model's workgroup publishes them as the layer-0 panels of the wgrad launch, and no d(enc) is formed.
// Wide actions (PPOAF_ICM_WIDE_ACTIONS in n_action_slices, Discrete / Box with 9 <= max(A, A_in) <= 24): a third form of the
// models kernel, icm_sh_models_kernel<., 32>, and a second of the reward kernel, over a 32-column action tile (ShForm); the
// panels oI / aF of the wgrad launch are [Bpad][32].  A launch with A, A_in <= 8 or with slices runs the kernel it ran before.
#include "icm_update_dev.hpp"
#include "wgrad_tile.hpp"
#include <cstddef>

namespace ppoaf {

struct IcmSh {
    IcmDev d;                  // d.H = D (the forward loss's mean and the bookkeeping run over B x D); d.actE: hidden planes
    int E, D, DP, Mi, Mf;      // DP = pad16(D)
    int ident;                 // identity encoder: E = 0, D = O; enc is filled by the models kernel, gI / gF / dEh / dEo unused
    int n_sl;                  // MultiDiscrete: k >= 2 equal action slices of A / k classes (args->n_action_slices); else 0
    int wide;                  // host only: the 32-column action form (ShForm<32>) runs; fills the padding ahead of `enc`
    float* enc;                // [2][Bpad][DP]     encodings of the two streams
    float* gI;                 // [2][Bpad][DP]     the inverse model's share of d(enc_1), d(enc_2)
    float* gF;                 // [2][Bpad][DP]     the forward model's
    // panels of the wgrad launch (workspace); planeE = Bpad * E, planeI = Bpad * Mi, planeF = Bpad * Mf
    float* dEh;                // [2][3][planeE]    dz of encoder layers 0..2, stream-major
    float* dEo;                // [2][Bpad][DP]     dz of encoder layer 3 = d(enc)
    float* dFo;                // [Bpad][DP]        dz of the forward model's output layer
    // d.xO [2][Bpad][XO]; d.hI / d.dI [d_inv][planeI]; d.oI [Bpad][16]; d.hF / d.dF [d_fwd][planeF]; d.aF [Bpad][16]
    // (wide: d.oI and d.aF [Bpad][32])
};

static_assert(offsetof(IcmSh, enc) == sizeof(IcmDev) + 32, "IcmSh: `wide` sits in what was padding, the kernel arguments keep their layout");

extern __shared__ __attribute__((aligned(16))) unsigned char icm_sh_smem[];

constexpr int kShXS = 20;      // row stride of the padded action tile [16, 16 + 4]
constexpr int kShWideA = 24;   // classes / dimensions the 32-column form's head is written for (fused_update.WIDE_HEAD_MAX)

// The action-tile form of a models / reward kernel, from AW = the columns the inverse head is instantiated with.  8 and 16
// share the 16-column tile; 32 is the wide form: every size below is a compile-time constant of the instantiation.
template <int AW>
struct ShForm {
    static constexpr bool wide = AW == 32;
    static constexpr int XW = wide ? 32 : 16;               // columns of the action tile and of the panels oI / aF
    static constexpr int XSH = wide ? 5 : 4;                // log2(XW)
    static constexpr int XS = wide ? 36 : kShXS;            // row stride of the action tile [16][XW + 4]
    static constexpr int AS = wide ? 32 : 8;                // row stride of sAct
    static constexpr int OS = wide ? 32 : kMaxOut;          // row stride of sOut / sDOut
    static constexpr int HEAD = wide ? kShWideA : AW;       // columns the head and the output layer's backward run over
    static constexpr int kBout = 16 + kRows * AS;           // carve (floats): sRow [16] | sAct [16][AS] | sBout | sWout
    static constexpr int kWout = kBout + (wide ? 32 : 16);
};
static_assert(ShForm<8>::kBout == 144 && ShForm<8>::kWout == 160 && ShForm<16>::kWout == 160, "the narrow carve stays");
static_assert(ShForm<32>::kBout == 528 && ShForm<32>::kWout == 560, "the wide carve");

// ---- run-time sized MFMA tiles: weights by bound-checked scalar loads -------------------------------------------
// acc += A[16][K] . w[0..K) for this lane's output column; A in LDS (stride lda, readable and finite up to pad16(K))
__device__ __forceinline__ f32x4 sh_tile_fwd(f32x4 acc, const float* __restrict__ A, int lda, const float* __restrict__ w, int K,
                                             bool ok, int lane) {
    const float* arow = A + (lane & 15) * lda;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * j + (lane >> 4);
            bq[j] = (ok && k < K) ? w[k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
    }
    return acc;
}
// out[s][o] = f(bias[o] + sum_k A[s][k] W[o][k]) for o < n_out; columns n_out .. pad16(n_out) of `out` get zeros
__device__ __forceinline__ void sh_layer_fwd(const float* __restrict__ W, int ldw, const float* __restrict__ bias, int K, int n_out,
                                             const float* __restrict__ A, int lda, float* __restrict__ out, int ldo, int act,
                                             int wave, int lane) {
    for (int nt = wave; 16 * nt < n_out; nt += kNW) {
        const int o = nt * 16 + (lane & 15);
        const bool ok = o < n_out;
        const float bv = ok ? bias[o] : 0.f;
        f32x4 acc = {bv, bv, bv, bv};
        acc = sh_tile_fwd(acc, A, lda, W + (long)o * ldw, K, ok, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(4 * (lane >> 4) + r) * ldo + o] = !ok ? 0.f : (act >= 0 ? act_fwd(acc[r], act) : acc[r]);
    }
}
// dh[s][i] = (sum_o D[s][o] W[o][i]) * act'(Hin[s][i]) for i < n_in; columns n_in .. pad16(n_in) get zeros.  D in LDS
// (stride ldd, finite up to pad16(n_out)).  Result to LDS (dst_lds, stride ldo) or to global rows (dst_glob, stride ldo).
__device__ __forceinline__ void sh_layer_dgrad(const float* __restrict__ W, int ldw, int n_out, int n_in, const float* __restrict__ D,
                                               int ldd, const float* __restrict__ Hin, int ldh, int act, float* __restrict__ dst_lds,
                                               float* __restrict__ dst_glob, int ldo, int wave, int lane) {
    const float* drow = D + (lane & 15) * ldd;
    for (int nt = wave; 16 * nt < n_in; nt += kNW) {
        const int i = nt * 16 + (lane & 15);
        const bool ok = i < n_in;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < n_out; k0 += 16) {
            float bq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * j + (lane >> 4);
                bq[j] = (ok && k < n_out) ? W[(long)k * ldw + i] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(drow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = 4 * (lane >> 4) + r;
            float v = ok ? acc[r] : 0.f;
            if (ok && Hin) v *= act_bwd(Hin[s * ldh + i], act);
            if (dst_lds) dst_lds[s * ldo + i] = v;
            else dst_glob[(long)s * ldo + i] = v;
        }
    }
}
// 16 rows x n floats (n a multiple of 4) of LDS (row stride ls) -> rows [16 g, +16) of a [Bpad][n] panel, and back
__device__ __forceinline__ void sh_publish(const float* __restrict__ src, int ls, float* __restrict__ panel, int n, int g, int tid) {
    float* dst = panel + (long)g * kRows * n;
    const int n4 = n >> 2;
    for (int i = tid; i < kRows * n4; i += kThreadsU) {
        const int r = i / n4, c4 = i - r * n4;
        *reinterpret_cast<float4*>(dst + (long)r * n + 4 * c4) = *reinterpret_cast<const float4*>(src + r * ls + 4 * c4);
    }
}
__device__ __forceinline__ void sh_fetch(const float* __restrict__ panel, int n, int g, float* __restrict__ dst, int ls, int tid) {
    const float* src = panel + (long)g * kRows * n;
    const int n4 = n >> 2;
    for (int i = tid; i < kRows * n4; i += kThreadsU) {
        const int r = i / n4, c4 = i - r * n4;
        *reinterpret_cast<float4*>(dst + r * ls + 4 * c4) = *reinterpret_cast<const float4*>(src + (long)r * n + 4 * c4);
    }
}
// identity encoder: the tile's 16 observation rows (stride O floats: not 16-byte aligned in general, so one dword per
// lane, consecutive lanes on consecutive columns) -> dst [16][ls]; dead rows and columns O .. DP are written as zeros
__device__ __forceinline__ void sh_load_obs(const float* __restrict__ src, int O, int DP, const int* sRow, float* __restrict__ dst,
                                            int ls, int tid) {
    for (int idx = tid; idx < kRows * DP; idx += kThreadsU) {
        const int s = idx / DP, i = idx - s * DP;
        const int row = sRow[s];
        dst[s * ls + i] = (row >= 0 && i < O) ? src[(long)row * O + i] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// encoder forward: block 2 * g + which (0: obs, 1: next_obs)
// ------------------------------------------------------------------------------------------------
template <int ET>
__global__ __launch_bounds__(kThreadsU) void icm_sh_encoder_fwd_kernel(IcmSh q) {
    constexpr int E = 16 * ET, ES = E + 4;
    const IcmDev& u = q.d;
    const int vb = icm_block(u);
    if (vb < 0 || vb >= 2 * u.nT) return;
    const int which = vb & 1, g = vb >> 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int O = u.O, INP = 16 * ((O + 15) >> 4) + 4, D = q.D, DP = q.DP, DS = DP + 4;
    const float* P = u.params + u.enc_off;
    auto encW = [&](int l) -> long { return l == 0 ? 0 : (long)E * O + E + (long)(l - 1) * (E * E + E); };
    auto encB = [&](int l) -> long { return encW(l) + (l == 0 ? (long)E * O : (l < 3 ? (long)E * E : (long)D * E)); };
    float* smem = reinterpret_cast<float*>(icm_sh_smem);
    int* sRow = reinterpret_cast<int*>(smem);
    float* sX = smem + 16;                      // [16, INP]
    float* sH = sX + kRows * INP;               // 3 x [16, ES]
    float* sEnc = sH + 3L * kRows * ES;         // [16, DS]
    if (vb == 0 && tid == 0 && u.fused_adam) {
        // Adam step counter and the two bias-correction constants of this mini-batch, computed once (in double, as
        // torch.optim.Adam does) and parked behind the loss partials for the wgrad launch
        const int64_t t = u.step_count[0] + 1;
        u.step_count[0] = t;
        u.loss_partials[2 * u.nT] = (float)((double)u.lr[0] / (1.0 - pow((double)u.beta1, (double)t)));
        u.loss_partials[2 * u.nT + 1] = (float)sqrt(1.0 - pow((double)u.beta2, (double)t));
    }
    icm_rows(u, g, tid, sRow);
    for (int i = tid; i < kRows * INP; i += kThreadsU) sX[i] = 0.f;
    __syncthreads();
    {
        const float* src = which == 0 ? u.obs : u.next_obs;
        for (int idx = tid; idx < kRows * O; idx += kThreadsU) {
            const int s = idx / O, i = idx - s * O;
            const int row = sRow[s];
            if (row >= 0) sX[s * INP + i] = src[(long)row * O + i];
        }
    }
    __syncthreads();
    if (u.xO) {             // the layer-0 wgrad's K-panel: this tile's rows, zero padded to XO columns
        float* xo = u.xO + ((long)which * u.Bpad + (long)g * kRows) * u.XO;
        for (int i = tid; i < kRows * u.XO; i += kThreadsU) { const int r = i / u.XO, c = i - r * u.XO; xo[i] = sX[r * INP + c]; }
    }
    sh_layer_fwd(P + encW(0), O, P + encB(0), O, E, sX, INP, sH, ES, u.act, wave, lane);
    __syncthreads();
    layer_fwd<ET, true>(P + encW(1), E, P + encB(1), sH, sH + kRows * ES, u.act, wave, lane);
    __syncthreads();
    layer_fwd<ET, true>(P + encW(2), E, P + encB(2), sH + kRows * ES, sH + 2L * kRows * ES, u.act, wave, lane);
    __syncthreads();
    sh_layer_fwd(P + encW(3), E, P + encB(3), E, D, sH + 2L * kRows * ES, ES, sEnc, DS, -1, wave, lane);
    __syncthreads();
    for (int l = 0; l < 3; ++l) sh_publish(sH + (long)l * kRows * ES, ES, u.actE + (long)(which * 3 + l) * u.Bpad * E, E, g, tid);
    sh_publish(sEnc, DS, q.enc + (long)which * u.Bpad * DP, DP, g, tid);
}

// ------------------------------------------------------------------------------------------------
// the forward model's forward pass on one row tile, shared by the update and the reward kernel: sE1 [16][DS] and
// sXa [16][XS] in, hidden planes in sH (depth x [16][MS]), the prediction of enc_2 in sPred [16][DS].  Ends with a barrier.
// ------------------------------------------------------------------------------------------------
template <int MT, int XS>
__device__ __forceinline__ void sh_forward_model(const IcmSh& q, const float* __restrict__ P, const float* sE1, const float* sXa,
                                                 float* sH, float* sPred, int wave, int lane) {
    constexpr int M = 16 * MT, MS = M + 4;
    const IcmDev& u = q.d;
    const int D = q.D, DS = q.DP + 4, Ain = u.Ain, depth = u.d_fwd, ld0 = D + Ain;
    auto offW = [&](int l) -> long { return l == 0 ? 0 : (long)M * ld0 + M + (long)(l - 1) * (M * M + M); };
    auto offB = [&](int l) -> long { return offW(l) + (l == 0 ? (long)M * ld0 : (l < depth ? (long)M * M : (long)D * M)); };
    for (int nt = wave; nt < MT; nt += kNW) {               // layer 0 over cat(enc_1, one-hot | action)
        const int o = nt * 16 + (lane & 15);
        const float bv = P[offB(0) + o];
        f32x4 acc = {bv, bv, bv, bv};
        acc = sh_tile_fwd(acc, sE1, DS, P + (long)o * ld0, D, true, lane);
        acc = sh_tile_fwd(acc, sXa, XS, P + (long)o * ld0 + D, Ain, true, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) sH[(4 * (lane >> 4) + r) * MS + o] = act_fwd(acc[r], u.act);
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l < depth; ++l) {
        layer_fwd<MT, true>(P + offW(l), M, P + offB(l), sH + (long)(l - 1) * kRows * MS, sH + (long)l * kRows * MS, u.act, wave, lane);
        __syncthreads();
    }
    sh_layer_fwd(P + offW(depth), M, P + offB(depth), M, D, sH + (long)(depth - 1) * kRows * MS, MS, sPred, DS, -1, wave, lane);
    __syncthreads();
}

// the action columns of a row tile: one-hot (icm.py:198-204), one one-hot per slice side by side (MultiDiscrete with equal
// class counts, icm.py:198-211) or the action values, zero padded; sAct keeps the class(es) / the values for the inverse
// model's loss.  A class outside its slice is clamped into it: nothing is read or set beyond the slice.
// XS / AS: row strides of sXa / sAct (ShForm).
template <int XS, int AS>
__device__ __forceinline__ void sh_actions(const IcmDev& u, int n_sl, const int* sRow, float* sAct, float* sXa, int tid) {
    if (tid < kRows) {
        const int row = sRow[tid], A = u.A;
        if (n_sl >= 2) {
            const int n = A / n_sl;
            for (int j = 0; j < n_sl; ++j) {
                int a = row >= 0 ? (int)reinterpret_cast<const int64_t*>(u.actions)[(long)row * n_sl + j] : 0;
                a = a < 0 ? 0 : (a >= n ? n - 1 : a);
                reinterpret_cast<int*>(sAct)[tid * AS + j] = a;
                if (row >= 0) sXa[tid * XS + j * n + a] = 1.0f;
            }
        } else if (u.discrete) {
            int a = row >= 0 ? (int)reinterpret_cast<const int64_t*>(u.actions)[row] : 0;
            a = a < 0 ? 0 : (a >= A ? A - 1 : a);
            reinterpret_cast<int*>(sAct)[tid * AS] = a;
            if (row >= 0) sXa[tid * XS + a] = 1.0f;
        } else {
            for (int d = 0; d < A; ++d) {
                const float v = row >= 0 ? reinterpret_cast<const float*>(u.actions)[(long)row * A + d] : 0.f;
                sAct[tid * AS + d] = v;
                sXa[tid * XS + d] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// models: block 2 * g + which (0: inverse model, 1: forward model); only >= 0: every block runs that model on tile
// blockIdx (the launch per model when the two widths differ).  AW: the columns the inverse model's head is written for.
// 8 is the Discrete / Box head (A <= 8); 16 the MultiDiscrete one (n_action_slices >= 2, A <= 16), an instantiation of its
// own so that the A <= 8 shapes keep their head's arithmetic and their 8-wide tiles (sh_actions is shared by both);
// 32 the wide Discrete / Box one (9 <= max(A, A_in) <= kShWideA) over the 32-column tile of ShForm<32>.
// ------------------------------------------------------------------------------------------------
template <int MT, int AW>
__global__ __launch_bounds__(kThreadsU) void icm_sh_models_kernel(IcmSh q, int only) {
    constexpr int M = 16 * MT, MS = M + 4;
    const IcmDev& u = q.d;
    const int vb = icm_block(u);
    if (vb < 0 || vb >= (only >= 0 ? u.nT : 2 * u.nT)) return;
    const int which = only >= 0 ? only : (vb & 1), g = only >= 0 ? vb : (vb >> 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int act = u.act, A = u.A, D = q.D, DP = q.DP, DS = DP + 4;
    const int depth = which == 0 ? u.d_inv : u.d_fwd;
    const long B = u.B;
    using F = ShForm<AW>;
    constexpr int XS = F::XS, AS = F::AS, OS = F::OS;
    float* smem = reinterpret_cast<float*>(icm_sh_smem);
    int* sRow = reinterpret_cast<int*>(smem);                 // [16]
    float* sAct = smem + 16;                                  // [16][AS] actions (float, or int bits)
    float* sBout = smem + F::kBout;                           // [16] (wide: [32])
    float* sWout = smem + F::kWout;                           // [AW, M]
    float* sXa = sWout + AW * M;                              // [16, XS]
    float* sE1 = sXa + kRows * XS;                            // [16, DS]
    float* sE2 = sE1 + kRows * DS;
    float* sP = sE2 + kRows * DS;                             // [16, DS]  forward model: prediction, then its dz
    float* sH = sP + kRows * DS;                              // depth x [16, MS]
    float* sD0 = sH + (long)depth * kRows * MS;
    float* sD1 = sD0 + kRows * MS;
    float* sOut = sD1 + kRows * MS;                           // [16, OS]
    float* sDOut = sOut + kRows * OS;                         // [16, OS]
    __shared__ float red[17];

    if (q.ident && vb == 0 && which == 0 && tid == 0 && u.fused_adam) {
        // (no encoder launch ahead of this one: the Adam constants of icm_sh_encoder_fwd_kernel are computed here)
        const int64_t t = u.step_count[0] + 1;
        u.step_count[0] = t;
        u.loss_partials[2 * u.nT] = (float)((double)u.lr[0] / (1.0 - pow((double)u.beta1, (double)t)));
        u.loss_partials[2 * u.nT + 1] = (float)sqrt(1.0 - pow((double)u.beta2, (double)t));
    }
    icm_rows(u, g, tid, sRow);
    for (int i = tid; i < kRows * XS; i += kThreadsU) sXa[i] = 0.f;
    if (q.ident) {
        __syncthreads();
        sh_load_obs(u.obs, u.O, DP, sRow, sE1, DS, tid);
        sh_load_obs(u.next_obs, u.O, DP, sRow, sE2, DS, tid);
    } else {
        sh_fetch(q.enc, DP, g, sE1, DS, tid);
        sh_fetch(q.enc + u.Bpad * DP, DP, g, sE2, DS, tid);
    }
    __syncthreads();
    sh_actions<XS, AS>(u, q.n_sl, sRow, sAct, sXa, tid);
    __syncthreads();
    if (q.ident && which == 0) {        // the layer-0 inputs of the wgrad launch
        sh_publish(sE1, DS, q.enc, DP, g, tid);
        sh_publish(sE2, DS, q.enc + u.Bpad * DP, DP, g, tid);
    }

    if (which == 0) {
        // =================================== inverse model ===================================
        const float* P = u.params + u.inv_off;
        const int ld0 = 2 * D;
        auto offW = [&](int l) -> long { return l == 0 ? 0 : (long)M * ld0 + M + (long)(l - 1) * (M * M + M); };
        auto offB = [&](int l) -> long { return offW(l) + (l == 0 ? (long)M * ld0 : (l < depth ? (long)M * M : (long)A * M)); };
        for (int i = tid; i < A * M; i += kThreadsU) sWout[i] = P[offW(depth) + i];
        if (tid < A) sBout[tid] = P[offB(depth) + tid];
        for (int nt = wave; nt < MT; nt += kNW) {           // layer 0 over the two K = D halves of cat(enc_1, enc_2)
            const int o = nt * 16 + (lane & 15);
            const float bv = P[offB(0) + o];
            f32x4 acc = {bv, bv, bv, bv};
            acc = sh_tile_fwd(acc, sE1, DS, P + (long)o * ld0, D, true, lane);
            acc = sh_tile_fwd(acc, sE2, DS, P + (long)o * ld0 + D, D, true, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) sH[(4 * (lane >> 4) + r) * MS + o] = act_fwd(acc[r], act);
        }
        __syncthreads();
#pragma unroll 1
        for (int l = 1; l < depth; ++l) {
            layer_fwd<MT, true>(P + offW(l), M, P + offB(l), sH + (long)(l - 1) * kRows * MS, sH + (long)l * kRows * MS, act, wave, lane);
            __syncthreads();
        }
        const float* Hlast = sH + (long)(depth - 1) * kRows * MS;
        for (int l = 0; l < depth; ++l) sh_publish(sH + (long)l * kRows * MS, MS, u.hI + (long)l * u.Bpad * M, M, g, tid);
        // output layer (A <= AW): VALU from LDS + 16-lane reductions
        if (tid < 256) {
            const int s = tid >> 4, part = tid & 15;
            for (int k = 0; k < A; ++k) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < MT; ++i) acc = fmaf(Hlast[s * MS + part + 16 * i], sWout[k * M + part + 16 * i], acc);
                acc = group16_sum(acc);
                if (part == 0) sOut[s * OS + k] = acc + sBout[k];
            }
        }
        __syncthreads();
        // loss + d(out)
        if (wave == 0) {
            const int s = lane;
            const bool live = s < kRows && sRow[s] >= 0;
            float part = 0.f;
            if constexpr (AW == 32) {
                // the wide Discrete / Box head: the 8-wide head's arithmetic over NH = 24 columns, one lane per row, classes in
                // ascending order; every per-class array has compile-time indices only (registers, no private segment)
                constexpr int NH = F::HEAD;
                if (live && u.discrete) {
                    // icm.py:76-77, 404-415: softmax output fed to CrossEntropyLoss (a second log-softmax with its own max)
                    float p[NH];
                    float m = -INFINITY;
#pragma unroll
                    for (int k = 0; k < NH; ++k) if (k < A) m = fmaxf(m, sOut[s * OS + k]);
                    float ssum = 0.f;
#pragma unroll
                    for (int k = 0; k < NH; ++k) { p[k] = k < A ? expf(sOut[s * OS + k] - m) : 0.f; ssum += p[k]; }
#pragma unroll
                    for (int k = 0; k < NH; ++k) p[k] /= ssum;
                    float m2 = -INFINITY;
#pragma unroll
                    for (int k = 0; k < NH; ++k) if (k < A) m2 = fmaxf(m2, p[k]);
                    float e2[NH], s2 = 0.f;
#pragma unroll
                    for (int k = 0; k < NH; ++k) { e2[k] = k < A ? expf(p[k] - m2) : 0.f; s2 += e2[k]; }
                    const int a = reinterpret_cast<const int*>(sAct)[s * AS];
                    float pa = 0.f;
#pragma unroll
                    for (int k = 0; k < NH; ++k) if (k == a) pa = p[k];
                    part = -(pa - m2 - logf(s2));
                    const float sc = u.icm_beta / (float)B;
                    float dq[NH], dot = 0.f;
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        dq[k] = k < A ? sc * (e2[k] / s2 - (k == a ? 1.f : 0.f)) : 0.f;
                        dot += dq[k] * p[k];
                    }
#pragma unroll
                    for (int k = 0; k < NH; ++k) sDOut[s * OS + k] = p[k] * (dq[k] - dot);
                } else if (live) {
                    // icm.py:417-419: mean squared error over B x A
                    const float sc = u.icm_beta * 2.0f / ((float)B * (float)A);
#pragma unroll
                    for (int k = 0; k < NH; ++k) {
                        float dv = 0.f;
                        if (k < A) {
                            const float diff = sOut[s * OS + k] - sAct[s * AS + k];
                            part += diff * diff;
                            dv = sc * diff;
                        }
                        sDOut[s * OS + k] = dv;
                    }
                } else if (s < kRows) {
#pragma unroll
                    for (int k = 0; k < NH; ++k) sDOut[s * OS + k] = 0.f;
                }
            } else if constexpr (AW == 16) {
                if (live) {
                    // icm.py:76-77, 400-412: ONE softmax p over the whole row, then per slice CrossEntropyLoss on p[slice]
                    // (a second log-softmax over the slice, with its own max); the row's loss is the sum over the slices
                    const int nsl = q.n_sl, n = A / nsl;
                    float p[16];
                    float m = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 16; ++k) if (k < A) m = fmaxf(m, sOut[s * kMaxOut + k]);
                    float ssum = 0.f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) { p[k] = k < A ? expf(sOut[s * kMaxOut + k] - m) : 0.f; ssum += p[k]; }
#pragma unroll
                    for (int k = 0; k < 16; ++k) p[k] /= ssum;
                    const float sc = u.icm_beta / (float)B;
                    float dq[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) dq[k] = 0.f;
#pragma unroll 1
                    for (int j = 0; j < nsl; ++j) {
                        const int lo = j * n, hi = lo + n;
                        const int a = lo + reinterpret_cast<const int*>(sAct)[s * 8 + j];
                        float m2 = -INFINITY;
#pragma unroll
                        for (int k = 0; k < 16; ++k) if (k >= lo && k < hi) m2 = fmaxf(m2, p[k]);
                        float e2[16], s2 = 0.f;
#pragma unroll
                        for (int k = 0; k < 16; ++k) { e2[k] = (k >= lo && k < hi) ? expf(p[k] - m2) : 0.f; s2 += e2[k]; }
                        float pa = 0.f;
#pragma unroll
                        for (int k = 0; k < 16; ++k) if (k == a) pa = p[k];
                        part += -(pa - m2 - logf(s2));
#pragma unroll
                        for (int k = 0; k < 16; ++k) if (k >= lo && k < hi) dq[k] = sc * (e2[k] / s2 - (k == a ? 1.f : 0.f));
                    }
                    float dot = 0.f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) dot += dq[k] * p[k];
#pragma unroll
                    for (int k = 0; k < 16; ++k) sDOut[s * kMaxOut + k] = p[k] * (dq[k] - dot);
                } else if (s < kRows) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) sDOut[s * kMaxOut + k] = 0.f;
                }
            } else if (live && u.discrete) {
                // icm.py:404-409: softmax output fed to CrossEntropyLoss (a second log-softmax)
                float p[8];
                float m = -INFINITY;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < A) m = fmaxf(m, sOut[s * kMaxOut + k]);
                float ssum = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) { p[k] = k < A ? expf(sOut[s * kMaxOut + k] - m) : 0.f; ssum += p[k]; }
#pragma unroll
                for (int k = 0; k < 8; ++k) p[k] /= ssum;
                float m2 = -INFINITY;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < A) m2 = fmaxf(m2, p[k]);
                float e2[8], s2 = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) { e2[k] = k < A ? expf(p[k] - m2) : 0.f; s2 += e2[k]; }
                const int a = reinterpret_cast<const int*>(sAct)[s * 8];
                float pa = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k == a) pa = p[k];
                part = -(pa - m2 - logf(s2));
                const float sc = u.icm_beta / (float)B;
                float dq[8], dot = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    dq[k] = k < A ? sc * (e2[k] / s2 - (k == a ? 1.f : 0.f)) : 0.f;
                    dot += dq[k] * p[k];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) sDOut[s * kMaxOut + k] = p[k] * (dq[k] - dot);
            } else if (live) {
                // icm.py:411-413: mean squared error over B x A
                const float sc = u.icm_beta * 2.0f / ((float)B * (float)A);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float dv = 0.f;
                    if (k < A) {
                        const float diff = sOut[s * kMaxOut + k] - sAct[s * 8 + k];
                        part += diff * diff;
                        dv = sc * diff;
                    }
                    sDOut[s * kMaxOut + k] = dv;
                }
            } else if (s < kRows) {
#pragma unroll
                for (int k = 0; k < 8; ++k) sDOut[s * kMaxOut + k] = 0.f;
            }
            float v = lane < kRows ? part : 0.f;
            v = group16_sum(v);
            if (lane == 0) u.loss_partials[g * 2 + 0] = v;
        }
        __syncthreads();
        // output layer backward
        if (tid < kRows * F::XW) {                              // d(out) rows, zero padded to XW columns
            const int s = tid >> F::XSH, k = tid & (F::XW - 1);
            u.oI[((long)g * kRows + s) * F::XW + k] = k < F::HEAD ? sDOut[s * OS + k] : 0.f;
        }
        if (tid >= 256) {
            const int t2 = tid - 256;
            const int s = t2 >> 4, ig = t2 & 15;
            float d[F::HEAD];
#pragma unroll
            for (int k = 0; k < F::HEAD; ++k) d[k] = sDOut[s * OS + k];
            float hv[MT], acc[MT];
#pragma unroll
            for (int ii = 0; ii < MT; ++ii) { hv[ii] = Hlast[s * MS + ig + 16 * ii]; acc[ii] = 0.f; }
#pragma unroll
            for (int k = 0; k < F::HEAD; ++k) {
                if (k < A) {
#pragma unroll
                    for (int ii = 0; ii < MT; ++ii) acc[ii] = fmaf(d[k], sWout[k * M + ig + 16 * ii], acc[ii]);
                }
            }
#pragma unroll
            for (int ii = 0; ii < MT; ++ii) sD0[s * MS + ig + 16 * ii] = acc[ii] * act_bwd(hv[ii], act);
        }
        __syncthreads();
        float* Dc = sD0;
        float* Dn = sD1;
#pragma unroll 1
        for (int l = depth - 1; l >= 1; --l) {
            layer_dgrad<MT>(P + offW(l), M, Dc, sH + (long)(l - 1) * kRows * MS, act, Dn, nullptr, wave, lane);
            sh_publish(Dc, MS, u.dI + (long)l * u.Bpad * M, M, g, tid);
            __syncthreads();
            float* t = Dc; Dc = Dn; Dn = t;
        }
        // layer 0: two K halves; the shares of the encodings' gradients leave through scratch
        sh_publish(Dc, MS, u.dI, M, g, tid);
        if (q.ident) return;            // observations take no gradient
        sh_layer_dgrad(P, ld0, M, D, Dc, MS, nullptr, 0, act, nullptr, q.gI + (long)g * kRows * DP, DP, wave, lane);
        sh_layer_dgrad(P + D, ld0, M, D, Dc, MS, nullptr, 0, act, nullptr, q.gI + (u.Bpad + (long)g * kRows) * DP, DP, wave, lane);
    } else {
        // =================================== forward model ===================================
        const float* P = u.params + u.fwd_off;
        const int ld0 = D + u.Ain;
        auto offW = [&](int l) -> long { return l == 0 ? 0 : (long)M * ld0 + M + (long)(l - 1) * (M * M + M); };
        sh_forward_model<MT, XS>(q, P, sE1, sXa, sH, sP, wave, lane);
        for (int l = 0; l < depth; ++l) sh_publish(sH + (long)l * kRows * MS, MS, u.hF + (long)l * u.Bpad * M, M, g, tid);
        if (tid < kRows * F::XW) {                              // the action columns of layer 0's input
            const int s = tid >> F::XSH, k = tid & (F::XW - 1);
            u.aF[((long)g * kRows + s) * F::XW + k] = sXa[s * XS + k];
        }
        // K8: f_loss = 0.5 mean((pred - enc_2)^2); d pred = (1 - beta) (pred - enc_2) / (B D); d enc_2 = -d pred
        {
            const float sc = (1.0f - u.icm_beta) / ((float)B * (float)D);
            float part = 0.f;
            float* dE2 = q.ident ? nullptr : q.gF + (u.Bpad + (long)g * kRows) * DP;
            for (int idx = tid; idx < kRows * DP; idx += kThreadsU) {
                const int s = idx / DP, i = idx - s * DP;
                float dv = 0.f;
                if (i < D && sRow[s] >= 0) {
                    const float diff = sP[s * DS + i] - sE2[s * DS + i];
                    part += diff * diff;
                    dv = sc * diff;
                }
                sP[s * DS + i] = dv;
                if (dE2) dE2[(long)s * DP + i] = -dv;
            }
            part = block_sum(part, red);
            if (tid == 0) u.loss_partials[g * 2 + 1] = 0.5f * part;
        }
        __syncthreads();
        sh_publish(sP, DS, q.dFo, DP, g, tid);
        // output layer backward, then the hidden layers
        sh_layer_dgrad(P + offW(depth), M, D, M, sP, DS, sH + (long)(depth - 1) * kRows * MS, MS, act, sD0, nullptr, MS, wave, lane);
        __syncthreads();
        float* Dc = sD0;
        float* Dn = sD1;
#pragma unroll 1
        for (int l = depth - 1; l >= 1; --l) {
            layer_dgrad<MT>(P + offW(l), M, Dc, sH + (long)(l - 1) * kRows * MS, act, Dn, nullptr, wave, lane);
            sh_publish(Dc, MS, u.dF + (long)l * u.Bpad * M, M, g, tid);
            __syncthreads();
            float* t = Dc; Dc = Dn; Dn = t;
        }
        sh_publish(Dc, MS, u.dF, M, g, tid);
        if (q.ident) return;
        sh_layer_dgrad(P, ld0, M, D, Dc, MS, nullptr, 0, act, nullptr, q.gF + (long)g * kRows * DP, DP, wave, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// rollout-time intrinsic reward: the forward model alone on the encodings icm_sh_encoder_fwd_kernel left (identity
// encoder: on the observation rows themselves, the only launch of the call);
// intr[row] = scale * sum_d (pred - enc_2)^2.  One workgroup per 16 rows.  AW: the action-tile form (ShForm; 8 or 32).
// ------------------------------------------------------------------------------------------------
template <int MT, int AW>
__global__ __launch_bounds__(kThreadsU) void icm_sh_reward_kernel(IcmSh q, float scale, float* __restrict__ intr_out) {
    const IcmDev& u = q.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x;
    if (g >= u.nT) return;
    const int DP = q.DP, DS = DP + 4;
    using F = ShForm<AW>;
    constexpr int XS = F::XS, AS = F::AS;
    float* smem = reinterpret_cast<float*>(icm_sh_smem);
    int* sRow = reinterpret_cast<int*>(smem);                 // [16]
    float* sAct = smem + 16;                                  // [16][AS]
    float* sXa = smem + F::kBout;                             // [16, XS]
    float* sE1 = sXa + kRows * XS;                            // [16, DS]
    float* sE2 = sE1 + kRows * DS;
    float* sP = sE2 + kRows * DS;
    float* sH = sP + kRows * DS;                              // d_fwd x [16, MS]
    icm_rows(u, g, tid, sRow);
    for (int i = tid; i < kRows * XS; i += kThreadsU) sXa[i] = 0.f;
    if (q.ident) {
        __syncthreads();
        sh_load_obs(u.obs, u.O, DP, sRow, sE1, DS, tid);
        sh_load_obs(u.next_obs, u.O, DP, sRow, sE2, DS, tid);
    } else {
        sh_fetch(q.enc, DP, g, sE1, DS, tid);
        sh_fetch(q.enc + u.Bpad * DP, DP, g, sE2, DS, tid);
    }
    __syncthreads();
    sh_actions<XS, AS>(u, q.n_sl, sRow, sAct, sXa, tid);
    __syncthreads();
    sh_forward_model<MT, XS>(q, u.params + u.fwd_off, sE1, sXa, sH, sP, wave, lane);
    // row sums of (pred - enc_2)^2: 16 lanes per row (columns D .. DP are zero on both sides)
    if (tid < 256) {
        const int s = tid >> 4, part = tid & 15;
        float acc = 0.f;
        for (int i = part; i < DP; i += 16) {
            const float d = sP[s * DS + i] - sE2[s * DS + i];
            acc = fmaf(d, d, acc);
        }
        acc = group16_sum(acc);
        const long row = (long)g * kRows + s;
        if (part == 0 && row < u.B) intr_out[row] = scale * acc;
    }
}

// ------------------------------------------------------------------------------------------------
// encoder backward: block 2 * g + which (0: obs, 1: next_obs)
// ------------------------------------------------------------------------------------------------
template <int ET>
__global__ __launch_bounds__(kThreadsU) void icm_sh_encoder_bwd_kernel(IcmSh q) {
    constexpr int E = 16 * ET, ES = E + 4;
    const IcmDev& u = q.d;
    const int vb = icm_block(u);
    if (vb < 0 || vb >= 2 * u.nT) return;
    const int which = vb & 1, g = vb >> 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int O = u.O, D = q.D, DP = q.DP, DS = DP + 4;
    const float* P = u.params + u.enc_off;
    auto encW = [&](int l) -> long { return l == 0 ? 0 : (long)E * O + E + (long)(l - 1) * (E * E + E); };
    float* smem = reinterpret_cast<float*>(icm_sh_smem);
    float* sH = smem;                           // 3 x [16, ES]
    float* sDe = sH + 3L * kRows * ES;          // [16, DS]
    float* sD0 = sDe + kRows * DS;              // [16, ES]
    float* sD1 = sD0 + kRows * ES;
    for (int l = 0; l < 3; ++l) sh_fetch(u.actE + (long)(which * 3 + l) * u.Bpad * E, E, g, sH + (long)l * kRows * ES, ES, tid);
    {
        // d(enc) of this stream: the inverse model's share, then the forward model's
        const float* a = q.gI + ((long)which * u.Bpad + (long)g * kRows) * DP;
        const float* b = q.gF + ((long)which * u.Bpad + (long)g * kRows) * DP;
        const int n4 = DP >> 2;
        for (int idx = tid; idx < kRows * n4; idx += kThreadsU) {
            const int s = idx / n4, c4 = idx - s * n4;
            const float4 va = *reinterpret_cast<const float4*>(a + (long)s * DP + 4 * c4);
            const float4 vb4 = *reinterpret_cast<const float4*>(b + (long)s * DP + 4 * c4);
            *reinterpret_cast<float4*>(sDe + s * DS + 4 * c4) = make_float4(va.x + vb4.x, va.y + vb4.y, va.z + vb4.z, va.w + vb4.w);
        }
    }
    __syncthreads();
    sh_publish(sDe, DS, q.dEo + (long)which * u.Bpad * DP, DP, g, tid);
    sh_layer_dgrad(P + encW(3), E, D, E, sDe, DS, sH + 2L * kRows * ES, ES, u.act, sD0, nullptr, ES, wave, lane);
    __syncthreads();
    float* Dc = sD0;
    float* Dn = sD1;
#pragma unroll 1
    for (int l = 2; l >= 1; --l) {
        layer_dgrad<ET>(P + encW(l), E, Dc, sH + (long)(l - 1) * kRows * ES, u.act, Dn, nullptr, wave, lane);
        sh_publish(Dc, ES, q.dEh + (long)(which * 3 + l) * u.Bpad * E, E, g, tid);
        __syncthreads();
        float* t = Dc; Dc = Dn; Dn = t;
    }
    sh_publish(Dc, ES, q.dEh + (long)(which * 3) * u.Bpad * E, E, g, tid);
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static long pad4l(long x) { return (x + 3) / 4 * 4; }
static bool sh_width(int w) { return w == 32 || w == 64 || w == 128; }
// n_action_slices = option bits above the slice count in the low byte (include/ppoaf_hip.h)
static bool sh_wide_bit(const ppoaf_icm_shapes_args_t* a) { return a->n_action_slices > 0 && (a->n_action_slices & PPOAF_ICM_WIDE_ACTIONS) != 0; }
static int sh_slices(const ppoaf_icm_shapes_args_t* a) { return sh_wide_bit(a) ? (a->n_action_slices & 0xff) : a->n_action_slices; }
// the 32-column action form runs: asked for, Discrete / Box, and a width the 16-column tile's head (A <= 8) does not take
static bool sh_wide(const ppoaf_icm_shapes_args_t* a) {
    return sh_wide_bit(a) && sh_slices(a) < 2 && (a->action_dim > 8 || a->fwd_action_dim > 8);
}

// topology and bucket layout only: what ppoaf_icm_shapes_check answers without a device
static int sh_check(const ppoaf_icm_shapes_args_t* a) {
    PPOAF_REQUIRE(a, "icm_shapes: null args");
    const bool ident = a->enc_hidden == 0;          // identity encoder: the encoding is the observation
    PPOAF_REQUIRE(ident || sh_width(a->enc_hidden), "icm_shapes: enc_hidden=%d is not an instantiated width (32, 64, 128)", a->enc_hidden);
    if (ident) {
        PPOAF_REQUIRE(a->enc_dim == a->obs_dim, "icm_shapes: enc_hidden=0 (identity encoder) needs enc_dim=%d to equal obs_dim=%d",
                      a->enc_dim, a->obs_dim);
        PPOAF_REQUIRE(a->obs_dim >= 1 && a->obs_dim <= 128, "icm_shapes: enc_hidden=0 (identity encoder): obs_dim=%d must be in [1,128]",
                      a->obs_dim);
    }
    PPOAF_REQUIRE(sh_width(a->inv_hidden) && sh_width(a->fwd_hidden),
                  "icm_shapes: inv_hidden=%d / fwd_hidden=%d are not instantiated widths (32, 64, 128)", a->inv_hidden, a->fwd_hidden);
    PPOAF_REQUIRE(a->enc_dim >= 1 && a->enc_dim <= 128, "icm_shapes: enc_dim=%d must be in [1,128]", a->enc_dim);
    PPOAF_REQUIRE(a->obs_dim >= 1 && a->obs_dim <= 1024, "icm_shapes: obs_dim=%d must be in [1,1024]", a->obs_dim);
    // (without the bit the word is a slice count, refused above 8 below: an option bit this library does not know is never
    // half-honoured)
    PPOAF_REQUIRE(!sh_wide_bit(a) || (a->n_action_slices & ~(PPOAF_ICM_WIDE_ACTIONS | 0xff)) == 0,
                  "icm_shapes: n_action_slices=0x%x carries option bits other than PPOAF_ICM_WIDE_ACTIONS (0x%x)", a->n_action_slices,
                  PPOAF_ICM_WIDE_ACTIONS);
    if (sh_slices(a) >= 2) {
        // MultiDiscrete over k equal slices (the agent-shared ICM of a MAT group): one class per slice in `actions`
        const int k = sh_slices(a);
        PPOAF_REQUIRE(a->discrete != 0, "icm_shapes: n_action_slices=%d needs discrete=1 (discrete=%d)", k, a->discrete);
        PPOAF_REQUIRE(a->action_dim == a->fwd_action_dim, "icm_shapes: n_action_slices=%d needs action_dim=%d to equal fwd_action_dim=%d",
                      k, a->action_dim, a->fwd_action_dim);
        PPOAF_REQUIRE(k <= 8, "icm_shapes: n_action_slices=%d must be at most 8", k);
        PPOAF_REQUIRE(a->action_dim >= 1 && a->action_dim <= 16, "icm_shapes: action_dim=%d must be in [1,16] with n_action_slices=%d",
                      a->action_dim, k);
        PPOAF_REQUIRE(a->action_dim % k == 0, "icm_shapes: action_dim=%d is not a multiple of n_action_slices=%d", a->action_dim, k);
        PPOAF_REQUIRE(a->action_dim / k >= 2, "icm_shapes: action_dim=%d / n_action_slices=%d leaves fewer than 2 classes per slice",
                      a->action_dim, k);
    } else if (sh_wide_bit(a)) {
        // PPOAF_ICM_WIDE_ACTIONS: Discrete / Box up to kShWideA classes or dimensions
        PPOAF_REQUIRE(a->action_dim >= 1 && a->action_dim <= kShWideA, "icm_shapes: action_dim=%d must be in [1,%d] with PPOAF_ICM_WIDE_ACTIONS",
                      a->action_dim, kShWideA);
        PPOAF_REQUIRE(a->fwd_action_dim >= 1 && a->fwd_action_dim <= kShWideA,
                      "icm_shapes: fwd_action_dim=%d must be in [1,%d] with PPOAF_ICM_WIDE_ACTIONS", a->fwd_action_dim, kShWideA);
        PPOAF_REQUIRE(!a->discrete || a->action_dim == a->fwd_action_dim,
                      "icm_shapes: discrete=%d needs action_dim=%d to equal fwd_action_dim=%d with PPOAF_ICM_WIDE_ACTIONS", a->discrete,
                      a->action_dim, a->fwd_action_dim);
    } else {
        PPOAF_REQUIRE(a->action_dim >= 1 && a->action_dim <= 8 && a->fwd_action_dim >= 1 && a->fwd_action_dim <= 8,
                      "icm_shapes: action_dim=%d fwd_action_dim=%d must be in [1,8]", a->action_dim, a->fwd_action_dim);
    }
    PPOAF_REQUIRE(a->depth_inv >= 1 && a->depth_inv <= 3 && a->depth_fwd >= 1 && a->depth_fwd <= 3,
                  "icm_shapes: hidden depths (%d, %d) out of [1,3]", a->depth_inv, a->depth_fwd);
    PPOAF_REQUIRE(a->activation >= 0 && a->activation <= 2, "icm_shapes: activation=%d", a->activation);
    PPOAF_REQUIRE(a->xcd_half >= 0 && a->xcd_half <= 2, "icm_shapes: xcd_half=%d (0, 1 or 2)", a->xcd_half);
    const long E = a->enc_hidden, D = a->enc_dim, Mi = a->inv_hidden, Mf = a->fwd_hidden, O = a->obs_dim, A = a->action_dim,
               Ain = a->fwd_action_dim;
    const long enc_size = ident ? 0 : E * O + E + 2 * (E * E + E) + D * E + pad4l(D);
    const long inv_size = Mi * 2 * D + Mi + (long)(a->depth_inv - 1) * (Mi * Mi + Mi) + A * Mi + pad4l(A);
    const long fwd_size = Mf * (D + Ain) + Mf + (long)(a->depth_fwd - 1) * (Mf * Mf + Mf) + D * Mf + pad4l(D);
    PPOAF_REQUIRE(a->enc_offset >= 0 && a->enc_offset % 4 == 0 && a->inv_offset == a->enc_offset + enc_size &&
                      a->fwd_offset == a->inv_offset + inv_size && a->bucket_total == a->fwd_offset + fwd_size,
                  "icm_shapes: bucket layout (enc %ld, inv %ld, fwd %ld, total %ld) does not match the topology "
                  "(sizes %ld, %ld, %ld)", (long)a->enc_offset, (long)a->inv_offset, (long)a->fwd_offset,
                  (long)a->bucket_total, enc_size, inv_size, fwd_size);
    return PPOAF_OK;
}

// panels of the wgrad launch in the workspace and its block table -> bytes
static size_t sh_layout(IcmSh& q, char* base, IcmWg* w) {
    IcmDev& u = q.d;
    const long E = q.E, DP = q.DP, Mi = q.Mi, Mf = q.Mf, Bp = u.Bpad;
    const long planeE = Bp * E, planeI = Bp * Mi, planeF = Bp * Mf, planeD = Bp * DP;
    size_t off = 0;
    auto take = [&](size_t floats) { float* p = reinterpret_cast<float*>(base + off); off += (floats * 4 + 255) & ~(size_t)255; return p; };
    u.XO = 16 * ((u.O + 15) / 16);
    const int pw = q.wide ? 32 : 16;          // columns of the action panels oI / aF (ShForm::XW)
    if (!q.ident) {
        u.xO = take((size_t)2 * Bp * u.XO);
        q.dEh = take((size_t)6 * planeE); q.dEo = take((size_t)2 * planeD);
    }
    u.hI = take((size_t)u.d_inv * planeI); u.dI = take((size_t)u.d_inv * planeI); u.oI = take((size_t)Bp * pw);
    u.hF = take((size_t)u.d_fwd * planeF); u.dF = take((size_t)u.d_fwd * planeF); q.dFo = take((size_t)planeD);
    u.aF = take((size_t)Bp * pw);
    if (!w) return off;
    w->n_blk = w->n_jobs = 0;
    const int Ei = (int)E, Di = q.D, DPi = (int)DP, Mii = (int)Mi, Mfi = (int)Mf;
    const long D = q.D;
    // encoder (both observation streams: two segments): layer 0 from the gathered rows, 1..2 from the hidden planes, 3 -> D
    // (identity encoder: no encoder blocks, 10 blocks at most)
    if (!q.ident) {
        long e = u.enc_off;
        icm_add_block(w, q.dEh, Ei, 3 * planeE, u.xO, u.XO, Bp * u.XO, 2, Ei, u.O, e, u.O, e + E * u.O);
        e += E * u.O + E;
        for (int l = 1; l < 3; ++l) {
            icm_add_block(w, q.dEh + l * planeE, Ei, 3 * planeE, u.actE + (l - 1) * planeE, Ei, 3 * planeE, 2, Ei, Ei, e, Ei, e + E * E);
            e += E * E + E;
        }
        icm_add_block(w, q.dEo, DPi, planeD, u.actE + 2 * planeE, Ei, 3 * planeE, 2, Di, Ei, e, Ei, e + D * E);
    }
    // inverse model: layer 0 as an enc_1 and an enc_2 block (columns 0 and D of rows of 2D), hidden layers, output layer
    long p = u.inv_off;
    icm_add_block(w, u.dI, Mii, 0, q.enc, DPi, 0, 1, Mii, Di, p, 2 * Di, p + Mi * 2 * D);
    icm_add_block(w, u.dI, Mii, 0, q.enc + planeD, DPi, 0, 1, Mii, Di, p + D, 2 * Di, -1);
    p += Mi * 2 * D + Mi;
    for (int l = 1; l < u.d_inv; ++l) {
        icm_add_block(w, u.dI + l * planeI, Mii, 0, u.hI + (l - 1) * planeI, Mii, 0, 1, Mii, Mii, p, Mii, p + Mi * Mi);
        p += Mi * Mi + Mi;
    }
    icm_add_block(w, u.oI, pw, 0, u.hI + (u.d_inv - 1) * planeI, Mii, 0, 1, u.A, Mii, p, Mii, p + (long)u.A * Mi);
    // forward model: layer 0 as an enc_1 and an action block, hidden layers, output layer (D rows)
    long f = u.fwd_off;
    const int ld0 = Di + u.Ain;
    icm_add_block(w, u.dF, Mfi, 0, q.enc, DPi, 0, 1, Mfi, Di, f, ld0, f + Mf * ld0);
    icm_add_block(w, u.dF, Mfi, 0, u.aF, pw, 0, 1, Mfi, u.Ain, f + D, ld0, -1);
    f += Mf * ld0 + Mf;
    for (int l = 1; l < u.d_fwd; ++l) {
        icm_add_block(w, u.dF + l * planeF, Mfi, 0, u.hF + (l - 1) * planeF, Mfi, 0, 1, Mfi, Mfi, f, Mfi, f + Mf * Mf);
        f += Mf * Mf + Mf;
    }
    icm_add_block(w, q.dFo, DPi, 0, u.hF + (u.d_fwd - 1) * planeF, Mfi, 0, 1, Di, Mfi, f, Mfi, f + D * Mf);
    static_assert(4 + 2 * (2 + 2 + 1) <= kIcmMaxBlk, "block table");
    icm_deal_jobs(w);
    return off;
}

static int make_sh(const ppoaf_icm_shapes_args_t* a, IcmSh& q, bool training) {
    int rc = sh_check(a);
    if (rc) return rc;
    PPOAF_REQUIRE(a->B >= 1 && a->B <= 65536 && a->batch_stride >= a->B, "icm_shapes: B=%ld stride=%ld (B in [1,65536])", (long)a->B,
                  (long)a->batch_stride);
    PPOAF_REQUIRE(a->params && a->obs && a->next_obs && a->actions && a->act_scratch, "icm_shapes: null pointer");
    PPOAF_REQUIRE(((uintptr_t)a->params & 15) == 0 && ((uintptr_t)a->act_scratch & 15) == 0,
                  "icm_shapes: buckets and scratch must be 16-byte aligned");
    if (training) {
        PPOAF_REQUIRE(a->grads && a->exp_avg && a->exp_avg_sq && a->step_count && a->lr && (a->perm || a->inputs_in_batch_order) &&
                          a->cursor && (a->denc_scratch || a->enc_hidden == 0) && a->loss_partials && a->totals && a->workspace,
                      "icm_shapes: null pointer (the workspace is mandatory: there is no slab form)");
        PPOAF_REQUIRE(((uintptr_t)a->grads & 15) == 0 && ((uintptr_t)a->exp_avg & 15) == 0 && ((uintptr_t)a->exp_avg_sq & 15) == 0 &&
                          ((uintptr_t)a->denc_scratch & 15) == 0 && ((uintptr_t)a->workspace & 255) == 0,
                      "icm_shapes: buckets and scratch must be 16-byte aligned, the workspace 256-byte aligned");
    }
    IcmDev& u = q.d;
    u = IcmDev();
    q.E = a->enc_hidden; q.D = a->enc_dim; q.DP = 16 * ((a->enc_dim + 15) / 16); q.Mi = a->inv_hidden; q.Mf = a->fwd_hidden;
    q.ident = a->enc_hidden == 0;
    q.n_sl = sh_slices(a) >= 2 ? sh_slices(a) : 0;
    q.wide = sh_wide(a);
    u.O = a->obs_dim; u.H = a->enc_dim; u.A = a->action_dim; u.Ain = a->fwd_action_dim;
    u.d_inv = a->depth_inv; u.d_fwd = a->depth_fwd; u.act = a->activation; u.discrete = a->discrete != 0;
    u.enc_off = a->enc_offset; u.inv_off = a->inv_offset; u.fwd_off = a->fwd_offset; u.enc_size = a->inv_offset - a->enc_offset;
    u.total = a->bucket_total;
    u.params = a->params; u.grads = a->grads; u.exp_avg = a->exp_avg; u.exp_avg_sq = a->exp_avg_sq; u.slabs = nullptr;
    u.step_count = a->step_count; u.lr = a->lr; u.beta1 = a->beta1; u.beta2 = a->beta2; u.adam_eps = a->adam_eps;
    u.grad_scale = a->grad_scale; u.obs = a->obs; u.next_obs = a->next_obs; u.actions = a->actions;
    u.perm = a->perm; u.row_map = a->row_map; u.n_rows = a->n_rows; u.cursor = a->cursor; u.B = a->B;
    u.batch_stride = a->batch_stride;
    u.nT = (int)((a->B + kRows - 1) / kRows);
    u.Bpad = (long)u.nT * kRows;
    u.icm_beta = a->icm_beta; u.fused_adam = training && a->fused_adam != 0; u.pregathered = a->inputs_in_batch_order != 0;
    u.actE = a->act_scratch; u.loss_partials = a->loss_partials; u.totals = a->totals;
    u.confine = training ? a->xcd_half : 0;
    u.split = training ? 1 : 0;
    q.enc = a->act_scratch + 6 * u.Bpad * q.E;      // (identity encoder: E = 0, the encodings are all of act_scratch)
    q.gI = q.gF = q.dEh = q.dEo = q.dFo = nullptr;
    if (training) {
        if (!q.ident) {
            q.gI = a->denc_scratch;
            q.gF = a->denc_scratch + 2 * u.Bpad * q.DP;
        }
        const size_t need = sh_layout(q, reinterpret_cast<char*>(a->workspace), nullptr);
        PPOAF_REQUIRE((size_t)a->workspace_bytes >= need, "icm_shapes: workspace of %ld B, %zu needed", (long)a->workspace_bytes, need);
    }
    return PPOAF_OK;
}

constexpr size_t kShMaxLds = 160 * 1024;      // gfx950: LDS per CU
static size_t sh_lds_enc_fwd(const IcmSh& q) {
    const size_t ES = q.E + 4, INP = 16 * ((q.d.O + 15) / 16) + 4, DS = q.DP + 4;
    return (16 + kRows * INP + 3 * kRows * ES + kRows * DS) * 4;
}
static size_t sh_lds_enc_bwd(const IcmSh& q) {
    const size_t ES = q.E + 4, DS = q.DP + 4;
    return (5 * kRows * ES + kRows * DS) * 4;
}
template <int AW>
static size_t sh_lds_models(const IcmSh& q, int M, int depth) {
    using F = ShForm<AW>;
    const size_t MS = M + 4, DS = q.DP + 4;
    return (F::kWout + (size_t)AW * M + kRows * F::XS + 3 * kRows * DS + (size_t)(depth + 2) * kRows * MS + 2 * kRows * F::OS) * 4;
}
template <int AW>
static size_t sh_lds_reward(const IcmSh& q) {
    using F = ShForm<AW>;
    const size_t MS = q.Mf + 4, DS = q.DP + 4;
    return (F::kBout + kRows * F::XS + 3 * kRows * DS + (size_t)q.d.d_fwd * kRows * MS) * 4;
}

template <int ET>
static int launch_sh_encoder(const IcmSh& q, bool backward, hipStream_t s) {
    const IcmDev& u = q.d;
    static bool big_f = false, big_b = false;
    const size_t lds = backward ? sh_lds_enc_bwd(q) : sh_lds_enc_fwd(q);
    const void* k = backward ? reinterpret_cast<const void*>(icm_sh_encoder_bwd_kernel<ET>) : reinterpret_cast<const void*>(icm_sh_encoder_fwd_kernel<ET>);
    const int rc = allow_large_lds(k, lds, backward ? big_b : big_f, backward ? "icm_sh_encoder_bwd" : "icm_sh_encoder_fwd");
    if (rc) return rc;
    const unsigned grid = u.confine ? 8u * (unsigned)((2 * u.nT + 3) / 4) : 2u * (unsigned)u.nT;
    if (backward) hipLaunchKernelGGL(icm_sh_encoder_bwd_kernel<ET>, dim3(grid), dim3(kThreadsU), lds, s, q);
    else hipLaunchKernelGGL(icm_sh_encoder_fwd_kernel<ET>, dim3(grid), dim3(kThreadsU), lds, s, q);
    return check_launch(backward ? "icm_sh_encoder_bwd" : "icm_sh_encoder_fwd");
}
static int launch_sh_encoder(const IcmSh& q, bool backward, hipStream_t s) {
    if (q.E == 32) return launch_sh_encoder<2>(q, backward, s);
    if (q.E == 64) return launch_sh_encoder<4>(q, backward, s);
    return launch_sh_encoder<8>(q, backward, s);
}

// only < 0: both models in one launch (the widths agree); else the launch of model `only`
template <int MT, int AW>
static int launch_sh_models(const IcmSh& q, int only, hipStream_t s) {
    const IcmDev& u = q.d;
    static bool big = false;
    const int dmax = only < 0 ? (u.d_inv > u.d_fwd ? u.d_inv : u.d_fwd) : (only == 0 ? u.d_inv : u.d_fwd);
    // widest case (M 128, D 128, depth 3): AW 16 19936 floats = 79744 B; AW 32 23152 floats = 92608 B
    const size_t lds = sh_lds_models<AW>(q, 16 * MT, dmax);
    PPOAF_REQUIRE(lds <= kShMaxLds, "icm_shapes: the models kernel needs %zu B of LDS (> 160 KiB)", lds);      // (sh_check: A <= AW)
    const int rc = allow_large_lds(reinterpret_cast<const void*>(icm_sh_models_kernel<MT, AW>), lds, big, "icm_sh_models");
    if (rc) return rc;
    const int n = only < 0 ? 2 * u.nT : u.nT;
    const unsigned grid = u.confine ? 8u * (unsigned)((n + 3) / 4) : (unsigned)n;
    hipLaunchKernelGGL((icm_sh_models_kernel<MT, AW>), dim3(grid), dim3(kThreadsU), lds, s, q, only);
    return check_launch("icm_sh_models");
}
template <int MT>
static int launch_sh_models(const IcmSh& q, int only, hipStream_t s) {
    if (q.wide) return launch_sh_models<MT, 32>(q, only, s);
    return q.n_sl >= 2 ? launch_sh_models<MT, 16>(q, only, s) : launch_sh_models<MT, 8>(q, only, s);
}
static int launch_sh_models(const IcmSh& q, int M, int only, hipStream_t s) {
    if (M == 32) return launch_sh_models<2>(q, only, s);
    if (M == 64) return launch_sh_models<4>(q, only, s);
    return launch_sh_models<8>(q, only, s);
}

template <int MT, int AW>
static int launch_sh_reward(const IcmSh& q, float scale, float* intr_out, hipStream_t s) {
    static bool big = false;
    // widest case (Mf 128, D 128, depth 3): 13136 floats = 52544 B; wide tile 13776 floats = 55104 B
    const size_t lds = sh_lds_reward<AW>(q);
    PPOAF_REQUIRE(lds <= kShMaxLds, "icm_shapes: the reward kernel needs %zu B of LDS (> 160 KiB)", lds);
    const int rc = allow_large_lds(reinterpret_cast<const void*>(icm_sh_reward_kernel<MT, AW>), lds, big, "icm_sh_reward");
    if (rc) return rc;
    hipLaunchKernelGGL((icm_sh_reward_kernel<MT, AW>), dim3((unsigned)q.d.nT), dim3(kThreadsU), lds, s, q, scale, intr_out);
    return check_launch("icm_sh_reward");
}
template <int MT>
static int launch_sh_reward(const IcmSh& q, float scale, float* intr_out, hipStream_t s) {
    return q.wide ? launch_sh_reward<MT, 32>(q, scale, intr_out, s) : launch_sh_reward<MT, 8>(q, scale, intr_out, s);
}

// the layouts the ctypes structure of _lib.py restates (tests/test_icm_shapes_scope.py reads this list)
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, obs_dim, 0);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, activation, 36);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, xcd_half, 44);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, enc_offset, 48);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, bucket_total, 72);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, params, 80);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, step_count, 112);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, beta1, 128);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, obs, 144);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, perm, 168);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, cursor, 192);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, icm_beta, 216);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, act_scratch, 224);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, loss_partials, 240);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, inputs_in_batch_order, 256);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, n_action_slices, 260);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, workspace, 264);
PPOAF_LAYOUT(ppoaf_icm_shapes_args_t, workspace_bytes, 272);
static_assert(sizeof(ppoaf_icm_shapes_args_t) == 280, "ppoaf_icm_shapes_args_t");

}  // namespace ppoaf

using namespace ppoaf;

extern "C" int ppoaf_icm_shapes_check(const ppoaf_icm_shapes_args_t* args) { return sh_check(args); }

extern "C" int ppoaf_icm_shapes_workspace_bytes(const ppoaf_icm_shapes_args_t* args, int64_t* bytes_out) {
    PPOAF_REQUIRE(args && bytes_out, "icm_shapes_workspace_bytes: null argument");
    const int rc = sh_check(args);
    if (rc) return rc;
    PPOAF_REQUIRE(args->B >= 1 && args->B <= 65536, "icm_shapes: B=%ld (B in [1,65536])", (long)args->B);
    IcmSh q;
    q.d = IcmDev();
    q.E = args->enc_hidden; q.D = args->enc_dim; q.DP = 16 * ((args->enc_dim + 15) / 16); q.Mi = args->inv_hidden; q.Mf = args->fwd_hidden;
    q.ident = args->enc_hidden == 0;
    q.wide = sh_wide(args);
    q.d.O = args->obs_dim; q.d.d_inv = args->depth_inv; q.d.d_fwd = args->depth_fwd;
    q.d.Bpad = (args->B + kRows - 1) / kRows * kRows;
    *bytes_out = (int64_t)sh_layout(q, nullptr, nullptr);
    return PPOAF_OK;
}

extern "C" int ppoaf_icm_shapes_fwd_bwd(const ppoaf_icm_shapes_args_t* args, ppoaf_stream_t stream) {
    IcmSh q;
    int rc = make_sh(args, q, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!q.ident) {
        PPOAF_REQUIRE(sh_lds_enc_fwd(q) <= 160 * 1024, "icm_shapes: the encoder needs %zu B of LDS (> 160 KiB)", sh_lds_enc_fwd(q));
        rc = launch_sh_encoder(q, false, s);
        if (rc) return rc;
    }
    if (q.Mi == q.Mf) rc = launch_sh_models(q, q.Mi, -1, s);
    else {
        rc = launch_sh_models(q, q.Mi, 0, s);
        if (!rc) rc = launch_sh_models(q, q.Mf, 1, s);
    }
    if (rc || q.ident) return rc;
    return launch_sh_encoder(q, true, s);
}

extern "C" int ppoaf_icm_shapes_wgrad(const ppoaf_icm_shapes_args_t* args, ppoaf_stream_t stream) {
    IcmSh q;
    const int rc = make_sh(args, q, true);
    if (rc) return rc;
    IcmWg w;
    sh_layout(q, reinterpret_cast<char*>(args->workspace), &w);
    return icm_launch_wgrad(q.d, w, (hipStream_t)stream);
}

extern "C" int ppoaf_icm_shapes_intrinsic_reward(const ppoaf_icm_shapes_args_t* args, float scale, float* intr_out,
                                                 ppoaf_stream_t stream) {
    IcmSh q;
    int rc = make_sh(args, q, false);
    if (rc) return rc;
    PPOAF_REQUIRE(intr_out, "icm_shapes_intrinsic_reward: null output");
    PPOAF_REQUIRE(args->perm == nullptr && args->fused_adam == 0 && args->inputs_in_batch_order == 0,
                  "icm_shapes_intrinsic_reward: rows are the batch itself (perm NULL, fused_adam 0, inputs_in_batch_order 0)");
    hipStream_t s = (hipStream_t)stream;
    if (!q.ident) {
        PPOAF_REQUIRE(sh_lds_enc_fwd(q) <= 160 * 1024, "icm_shapes: the encoder needs %zu B of LDS (> 160 KiB)", sh_lds_enc_fwd(q));
        rc = launch_sh_encoder(q, false, s);
        if (rc) return rc;
    }
    if (q.Mf == 32) return launch_sh_reward<2>(q, scale, intr_out, s);
    if (q.Mf == 64) return launch_sh_reward<4>(q, scale, intr_out, s);
    return launch_sh_reward<8>(q, scale, intr_out, s);
}
