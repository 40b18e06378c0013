// Device code that the MAT kernels K15 (update), K16 (rollout step) and K20 (evaluation step) of mat_update.hip share: the
// parameter list and tile constants, the [16, 64] tile primitives, the LDS carve (MatCtxT, MAT_TILES), the panel
// publishers and the encoder / decoder forward passes.
#pragma once
#include "mlp_device.hpp"

namespace ppoaf {

constexpr int kMD = 64;            // embedding width
constexpr int kMHS = kMD + 4;      // LDS row stride of a [16, 64] tile
constexpr int kMNW = 4;            // waves per workgroup
constexpr int kMT = 64 * kMNW;
constexpr int kMXS = 20;           // row stride of the action-token tile [16, 16 + 4]
constexpr int kMTile = kRows * kMHS;

// parameter tensors of MATActorCritic in module order (== bucket order); offsets in floats
enum MatP {
    A_ENC_W, A_LN_G, A_LN_B, A_LN1_G, A_LN1_B, A_LN2_G, A_LN2_B, A_LN3_G, A_LN3_B,
    A_K1_W, A_K1_B, A_Q1_W, A_Q1_B, A_V1_W, A_V1_B, A_P1_W, A_P1_B,
    A_K2_W, A_K2_B, A_Q2_W, A_Q2_B, A_V2_W, A_V2_B, A_P2_W, A_P2_B,
    A_M1_W, A_M1_B, A_M2_W, A_M2_B, A_H1_W, A_H1_B, A_HLN_G, A_HLN_B, A_H2_W, A_H2_B,
    C_OLN_G, C_OLN_B, C_ENC_W, C_ENC_B, C_LN_G, C_LN_B, C_LN1_G, C_LN1_B, C_LN2_G, C_LN2_B,
    C_K_W, C_K_B, C_Q_W, C_Q_B, C_V_W, C_V_B, C_P_W, C_P_B,
    C_M1_W, C_M1_B, C_M2_W, C_M2_B, C_H1_W, C_H1_B, C_HLN_G, C_HLN_B, C_H2_W, C_H2_B,
    MAT_NUM_PARAMS
};
static_assert(MAT_NUM_PARAMS == 63, "offset table layout");

// the panels of the split-wgrad chain that hold the inputs of the 18 linears (mat_update.hip: PPOAF_MAT_LIN_X)
enum MatX { X_X3, X_GAM, X_X2, X_AY2, X_ENC, X_X1, X_AY1, X_X0, X_GCM, X_H1, X_CY, X_H0, MAT_NUM_XPANELS };

// Diagnostic build only (-DPPOAF_MAT_STAMPS, tools/mat_stamps.py): s_memtime of workgroup 0 / thread 0 at the marked points
// of the update kernel, into a buffer nothing else reads.  The shipped library executes no stamp.
#ifdef PPOAF_MAT_STAMPS
static __device__ unsigned long long g_mat_stamps[64];
#define MAT_STAMP(k)                                                                     \
    do {                                                                                 \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                                       \
            unsigned long long t_;                                                       \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");    \
            g_mat_stamps[k] = t_;                                                        \
        }                                                                                \
    } while (0)
#else
#define MAT_STAMP(k) do {} while (0)
#endif

// ------------------------------------------------------------------------------------------------
// element-wise passes over a [16, 64] tile: thread = (row = tid >> 4, lane16 = tid & 15), 4 columns each
// ------------------------------------------------------------------------------------------------
// Exact (erf) GELU, nn.GELU's default (multi_agent_transformer.py:51-60).  erf by Abramowitz & Stegun 7.1.26 --
// erf(x) = 1 - (a1 t + .. + a5 t^5) exp(-x^2), t = 1 / (1 + p x), |error| <= 1.5e-7 -- instead of the library erff:
// one exponential (the SAME exp(-z^2 / 2) the derivative's density term needs), one reciprocal and five FMAs against
// ~85 instructions per element; a GELU pass over a tile was 1400 of a phase's 1500 cycles (tools/mat_stamps.py) and 16 of
// the kernel's 71 phases contain one.  1.5e-7 absolute on erf is 25 x below the 1e-5 parity tolerance of every output.
__device__ __forceinline__ void gelu_parts(float z, float& cdf, float& pdf) {
    const float x = fabsf(z) * 0.70710678118654752440f;
    const float e = __expf(-x * x);                            // = exp(-z^2 / 2)
    const float t = __frcp_rn(fmaf(0.3275911f, x, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float erf_abs = 1.0f - poly * t * e;
    cdf = 0.5f * (1.0f + copysignf(erf_abs, z));
    pdf = e * 0.39894228040143267794f;
}
__device__ __forceinline__ float gelu_f(float z) { float cdf, pdf; gelu_parts(z, cdf, pdf); return z * cdf; }
__device__ __forceinline__ float gelu_d(float z) { float cdf, pdf; gelu_parts(z, cdf, pdf); return cdf + z * pdf; }

// out = gelu(Z)
__device__ __forceinline__ void tile_gelu(const float* __restrict__ Z, float* __restrict__ out, int tid) {
    const int row = tid >> 4, l = tid & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[row * kMHS + l + 16 * j] = gelu_f(Z[row * kMHS + l + 16 * j]);
}
// D *= gelu'(Z)
__device__ __forceinline__ void tile_gelu_bwd(float* __restrict__ D, const float* __restrict__ Z, int tid) {
    const int row = tid >> 4, l = tid & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) D[row * kMHS + l + 16 * j] *= gelu_d(Z[row * kMHS + l + 16 * j]);
}
// out = A + B
__device__ __forceinline__ void tile_add(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out, int tid) {
    const int row = tid >> 4, l = tid & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[row * kMHS + l + 16 * j] = A[row * kMHS + l + 16 * j] + B[row * kMHS + l + 16 * j];
}
// Y = Xhat * g + b   (LayerNorm output re-materialised for the backward)
__device__ __forceinline__ void tile_affine(const float* __restrict__ Xhat, const float* __restrict__ g,
                                            const float* __restrict__ b, float* __restrict__ Y, int tid) {
    const int row = tid >> 4, l = tid & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = l + 16 * j; Y[row * kMHS + c] = Xhat[row * kMHS + c] * g[c] + b[c]; }
}

// LayerNorm over W <= 64 columns (tile stride `ld`): Xhat, rstd[16], Y = Xhat * g + b.  X may alias Y.
__device__ __forceinline__ void tile_ln_fwd(const float* X, int ld, int W, const float* __restrict__ g,
                                            const float* __restrict__ b, float* __restrict__ Xhat,
                                            float* __restrict__ rstd, float* Y, int tid) {
    const int row = tid >> 4, l = tid & 15;
    float x[4], s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = l + 16 * j; x[j] = c < W ? X[row * ld + c] : 0.f; s += x[j]; }
    const float mean = group16_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int c = l + 16 * j; x[j] = c < W ? x[j] - mean : 0.f; q += x[j] * x[j]; }
    const float rs = 1.0f / sqrtf(group16_sum(q) / (float)W + 1e-5f);
    if (l == 0) rstd[row] = rs;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = l + 16 * j;
        if (c < W) {
            const float xh = x[j] * rs;
            Xhat[row * ld + c] = xh;
            Y[row * ld + c] = xh * g[c] + b[c];
        }
    }
}
// LayerNorm backward: DX = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)); d gamma / d beta column sums -> slab.
// DX must not alias DY (the column sums read DY while the rows are being written).  DX == nullptr: no input gradient.
__device__ __forceinline__ void tile_ln_bwd(const float* __restrict__ DY, int ld, int W, const float* __restrict__ Xhat,
                                            const float* __restrict__ rstd, const float* __restrict__ g,
                                            float* __restrict__ DX, float* __restrict__ slab_g, float* __restrict__ slab_b,
                                            int tid) {
    const int row = tid >> 4, l = tid & 15;
    if (DX) {
        float dxh[4], xh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = l + 16 * j;
            xh[j] = c < W ? Xhat[row * ld + c] : 0.f;
            dxh[j] = c < W ? DY[row * ld + c] * g[c] : 0.f;
            s1 += dxh[j]; s2 += dxh[j] * xh[j];
        }
        const float m1 = group16_sum(s1) / (float)W, m2 = group16_sum(s2) / (float)W, rs = rstd[row];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int c = l + 16 * j; if (c < W) DX[row * ld + c] = (dxh[j] - m1 - xh[j] * m2) * rs; }
    }
    if (tid < 64) {
        if (tid < W) {
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) a = fmaf(DY[s * ld + tid], Xhat[s * ld + tid], a);
            slab_g[tid] = a;
        }
    } else if (tid < 128) {
        const int c = tid - 64;
        if (c < W) {
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) a += DY[s * ld + c];
            slab_b[c] = a;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// linears on [16, 64] tiles (one output tile of 16 columns per wave)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lin_fwd(const float* __restrict__ W, const float* __restrict__ bias,
                                        const float* __restrict__ A, float* __restrict__ out, int wave, int lane) {
    layer_fwd<4, true, kMNW>(W, kMD, bias, A, out, -1, wave, lane);
}
__device__ __forceinline__ void lin_wgrad(const float* __restrict__ Dt, const float* __restrict__ In,
                                          float* __restrict__ dW, float* __restrict__ dB, int wave, int lane, int tid) {
    layer_wgrad<4, kMNW>(Dt, In, kMHS, 4, kMD, dW, kMD, dB, wave, lane, tid);
}
// out (+)= Dt . W   (out must not alias Dt)
template <bool ACCUM>
__device__ __forceinline__ void lin_dgrad(const float* __restrict__ W, const float* __restrict__ Dt,
                                          float* __restrict__ out, int wave, int lane) {
    float4 fr[4];
    load_dgrad_frags_ld<4>(W, kMD, wave * 16, lane, fr);
    const f32x4 acc = mfma_rows_x_frags<4>(Dt, kMHS, lane, fr, 0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int idx = (4 * (lane >> 4) + r) * kMHS + wave * 16 + (lane & 15);
        out[idx] = ACCUM ? out[idx] + acc[r] : acc[r];
    }
}

// split-wgrad chain: a settled [16, 64] LDS tile -> rows [16 g, +16) of a [R][64] panel (one float4 per thread)
__device__ __forceinline__ void publish_tile(const float* __restrict__ T, float* __restrict__ panel, int g, int tid) {
    const int r = tid >> 4, c4 = tid & 15;
    *reinterpret_cast<float4*>(panel + ((long)g * kRows + r) * kMD + 4 * c4) =
        *reinterpret_cast<const float4*>(T + r * kMHS + 4 * c4);
}

// The same linears with their weight fragments REQUESTED AHEAD: a wave's share of a 64x64 linear is 4 float4 per lane (+ its
// bias element).  A phase of this kernel is a dependent chain -- barrier, weight fragments from the L2 (~400 cycles), A
// from LDS, 16 MFMAs (32 cycles each), LDS stores, barrier: ~1800 cycles by in-kernel stamps, tools/mat_stamps.py -- and
// the 400 cycles of fragment latency sit at the head of 45 of the 71 phases.  The update kernel therefore requests the
// fragments of the NEXT linear at the start of the phase that runs the current one (they land behind its MFMAs and the
// barrier).  Not deeper: vmcnt retires in order, so with a whole pass's fragments in flight every small load issued
// after them (LayerNorm gains, biases) waited for all of them -- measured slower than no prefetch at all.
struct MatFr { float4 f[4]; float b; };
__device__ __forceinline__ void pf_fwd(const float* __restrict__ W, const float* __restrict__ bias, int wave, int lane, MatFr& r) {
    load_fwd_frags_ld<4, true>(W, kMD, wave * 16, lane, r.f);
    r.b = bias[wave * 16 + (lane & 15)];
}
__device__ __forceinline__ void pf_dgrad(const float* __restrict__ W, int wave, int lane, MatFr& r) {
    load_dgrad_frags_ld<4>(W, kMD, wave * 16, lane, r.f);
    r.b = 0.f;
}
__device__ __forceinline__ void lin_fwd_r(const MatFr& r, const float* __restrict__ A, float* __restrict__ out, int wave, int lane) {
    const int o = wave * 16 + (lane & 15);
    const f32x4 acc = mfma_rows_x_frags<4>(A, kMHS, lane, r.f, r.b);
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(4 * (lane >> 4) + q) * kMHS + o] = acc[q];
}
template <bool ACCUM>
__device__ __forceinline__ void lin_dgrad_r(const MatFr& r, const float* __restrict__ Dt, float* __restrict__ out, int wave, int lane) {
    const f32x4 acc = mfma_rows_x_frags<4>(Dt, kMHS, lane, r.f, 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = (4 * (lane >> 4) + q) * kMHS + wave * 16 + (lane & 15);
        out[idx] = ACCUM ? out[idx] + acc[q] : acc[q];
    }
}

// ------------------------------------------------------------------------------------------------
// attention core on LDS tiles (K9's block-diagonal packing).  Q, K, V, Y, dY ... are [16, 64] tiles.
// ------------------------------------------------------------------------------------------------
// out[:, 16 nt ..] = A[16,16] . Z[:, 16 nt ..]; A from the 17-stride tile T, as is or transposed
__device__ __forceinline__ void att_a_times(const float* __restrict__ T, bool transposed, const float* __restrict__ Z,
                                            float* __restrict__ out, int nt, int lane) {
    const int i = lane & 15, slot = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kk = 4 * slot + j;
        const float a = transposed ? T[kk * 17 + i] : T[i * 17 + kk];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Z[kk * kMHS + 16 * nt + i], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(4 * slot + r) * kMHS + 16 * nt + i] = acc[r];
}
// One 16-wide K chunk of X Y^T (X, Y: [16, 64] tiles): the wave's share of a score tile
__device__ __forceinline__ f32x4 att_xyT_chunk(const float* __restrict__ X, const float* __restrict__ Y, int chunk, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float4 a = *reinterpret_cast<const float4*>(X + (lane & 15) * kMHS + 16 * chunk + 4 * (lane >> 4));
    const float4 b = *reinterpret_cast<const float4*>(Y + (lane & 15) * kMHS + 16 * chunk + 4 * (lane >> 4));
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}
// forward: probabilities -> sP (kept for the backward), Y = P V.  Three barriers inside, none after.
// The 16 x 16 score tile is ONE MFMA output tile: instead of one wave running its 16 dependent MFMAs and the softmax of all
// 16 rows while three waves wait (stamps: 3.6 k cycles per attention), every wave takes one 16-wide K chunk (4 MFMAs), the
// four partial tiles meet in LDS (the Y tile is free until the last phase), and every wave runs the softmax of 4 rows, one
// row per 16 lanes.
__device__ __forceinline__ void att_fwd(const float* Q, const float* K, const float* V, float* Y, float* sP,
                                        int L, int n_rows, bool masked, int wave, int lane) {
    {
        const f32x4 s = att_xyT_chunk(Q, K, wave, lane);
        const int col = lane & 15;
#pragma unroll
        for (int r = 0; r < 4; ++r) Y[wave * 272 + (4 * (lane >> 4) + r) * 17 + col] = s[r];
    }
    __syncthreads();
    {
        const int row = 4 * wave + (lane >> 4), col = lane & 15;
        const float sc = (Y[row * 17 + col] + Y[272 + row * 17 + col]) + (Y[544 + row * 17 + col] + Y[816 + row * 17 + col]);
        bool ok = row < n_rows && col < n_rows && (row / L) == (col / L);
        if (masked) ok = ok && (col % L) <= (row % L);
        const float x = ok ? sc * 0.125f : -INFINITY;                       // 1 / sqrt(64)
        const float m = group16_max(x);
        const float e = ok ? expf(x - m) : 0.f;
        const float den = group16_sum(e);
        sP[row * 17 + col] = den > 0.f ? e / den : 0.f;
    }
    __syncthreads();
    att_a_times(sP, false, V, Y, wave, lane);
}
// backward from dY: dQ, dK, dV (three distinct output tiles); sS is a 17-stride scratch tile; the partial tiles of
// dP = dY V^T meet in the dQ tile (written only in the last phase)
__device__ __forceinline__ void att_bwd(const float* Q, const float* K, const float* V, const float* sP, const float* dY,
                                        float* dQ, float* dK, float* dV, float* sS, int wave, int lane) {
    {
        const f32x4 dp = att_xyT_chunk(dY, V, wave, lane);
        const int col = lane & 15;
#pragma unroll
        for (int r = 0; r < 4; ++r) dQ[wave * 272 + (4 * (lane >> 4) + r) * 17 + col] = dp[r];
    }
    __syncthreads();
    {
        const int row = 4 * wave + (lane >> 4), col = lane & 15;
        const float dp = (dQ[row * 17 + col] + dQ[272 + row * 17 + col]) + (dQ[544 + row * 17 + col] + dQ[816 + row * 17 + col]);
        const float p = sP[row * 17 + col];
        const float dot = group16_sum(dp * p);
        sS[row * 17 + col] = p * (dp - dot) * 0.125f;
    }
    __syncthreads();
    att_a_times(sP, true, dY, dV, wave, lane);      // dV = P^T dY
    att_a_times(sS, false, K, dQ, wave, lane);      // dQ = dS K
    att_a_times(sS, true, Q, dK, wave, lane);       // dK = dS^T Q
}

// ------------------------------------------------------------------------------------------------
// narrow first layers (observation encoder K = O, action encoder K = Ain): weights [64, K] row-major
// ------------------------------------------------------------------------------------------------
// acc += X[:, 0 .. kend) . W[o, c0 .. c0 + kend)^T for the wave's 16 outputs o: X is a tile (stride ldx) whose column 0 is
// input column c0 of W's rows (stride Kdim, zero beyond it); k ascends, so chunks called in order are the unchunked chain
__device__ __forceinline__ void narrow_fwd_acc(const float* __restrict__ W, int Kdim, int c0, int kend,
                                               const float* __restrict__ X, int ldx, f32x4& acc, int wave, int lane) {
    const int o = wave * 16 + (lane & 15);
    const float* w = W + (long)o * Kdim + c0;
    const float* arow = X + (lane & 15) * ldx;
    for (int k0 = 0; k0 < kend; k0 += 16) {
        float bq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int k = k0 + 4 * j + (lane >> 4); bq[j] = c0 + k < Kdim ? w[k] : 0.f; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
    }
}
__device__ __forceinline__ void narrow_store(const f32x4& acc, float* __restrict__ out, int wave, int lane) {
    const int o = wave * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(4 * (lane >> 4) + r) * kMHS + o] = acc[r];
}
__device__ __forceinline__ void narrow_fwd(const float* __restrict__ W, int Kdim, const float* __restrict__ bias,
                                           const float* __restrict__ X, int ldx, float* __restrict__ out, int wave, int lane) {
    const float bv = bias ? bias[wave * 16 + (lane & 15)] : 0.f;
    f32x4 acc = {bv, bv, bv, bv};
    narrow_fwd_acc(W, Kdim, 0, Kdim, X, ldx, acc, wave, lane);
    narrow_store(acc, out, wave, lane);
}
// dX[16, n] = D[16,64] . W[64, 0 .. n) for rows of W of stride ldw (tile stride ldx; columns >= n untouched)
__device__ __forceinline__ void narrow_dgrad(const float* __restrict__ W, int ldw, int n, const float* __restrict__ Dt,
                                             float* __restrict__ dX, int ldx, int wave, int lane) {
    for (int nt = wave; nt * 16 < n; nt += kMNW) {
        const int i = nt * 16 + (lane & 15);
        float4 fr[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float* wp = W + (long)(16 * c + 4 * (lane >> 4)) * ldw + i;
            fr[c] = i < n ? make_float4(wp[0], wp[ldw], wp[2 * ldw], wp[3 * ldw]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const f32x4 acc = mfma_rows_x_frags<4>(Dt, kMHS, lane, fr, 0.f);
        if (i < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dX[(4 * (lane >> 4) + r) * ldx + i] = acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// narrow output layers (64 -> n_out <= 8) on the VALU
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void head_out_fwd(const float* __restrict__ W, const float* __restrict__ bias, int n_out,
                                             const float* __restrict__ Hh, float* __restrict__ sOut, int tid) {
    const int s = tid >> 4, part = tid & 15;
    for (int k = 0; k < n_out; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = fmaf(Hh[s * kMHS + part + 16 * i], W[k * kMD + part + 16 * i], acc);
        acc = group16_sum(acc);
        if (part == 0) sOut[s * 8 + k] = acc + bias[k];
    }
}
// dW[k][i], db[k] -> slab; dH[s][i] = sum_k dOut[s][k] W[k][i]
__device__ __forceinline__ void head_out_bwd(const float* __restrict__ W, int n_out, const float* __restrict__ Hh,
                                             const float* __restrict__ sDOut, float* __restrict__ dH,
                                             float* __restrict__ slabW, float* __restrict__ slabB, int tid) {
    if (tid < kMD) {
        float h[kRows];
#pragma unroll
        for (int s = 0; s < kRows; ++s) h[s] = Hh[s * kMHS + tid];
        for (int k = 0; k < n_out; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc = fmaf(sDOut[s * 8 + k], h[s], acc);
            slabW[k * kMD + tid] = acc;
        }
    } else if (tid < kMD + 8) {
        const int k = tid - kMD;
        float acc = 0.f;
        if (k < n_out)
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc += sDOut[s * 8 + k];
        if (k < ((n_out + 3) & ~3)) slabB[k] = acc;
    }
    const int s = tid >> 4, part = tid & 15;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n_out; ++k) {
        const float d = sDOut[s * 8 + k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(d, W[k * kMD + part + 16 * i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dH[s * kMHS + part + 16 * i] = acc[i];
}

// Barriers separate phases whose readers use a different thread <-> element mapping than the writers (MFMA
// tiles vs the 16-lanes-per-row passes).  Row-pass -> row-pass sequences (add -> LayerNorm, GELU -> LayerNorm,
// LayerNorm backward -> GELU backward) and accumulating dgrads into one tile touch only a thread's own elements
// and run without one.
#define MAT_SYNC() __syncthreads()

// tile indices: saved activations of the critic (0-11) and the actor (12-27), scratch (28-33)
enum { cZ1_ = 0, cN0_, cQ_, cK_, cV_, cY_, cN1_, cZM_, cN2_, cENC_, cZH_, cNH_,
       aZ_, aN0_, aQ1_, aK1_, aV1_, aY1_, aN1_, aK2_, aV2_, aQ2_, aY2_, aN2_, aZM_, aN3_, aZH_, aNH_,
       S0_, S1_, S2_, S3_, S4_, DENC_, MAT_NUM_TILES };

// Forward-only carve (K20): nothing is read back by a backward pass, so tiles whose lives never overlap share storage.
//   0 rep_enc (live through every decoder pass)   1-4 S0..S3   5 every pre-GELU tile (written by a linear, read by the
//   next phase's GELU)   6 / 7 / 8 q / k / v of the attention in flight   9 its y -- and every saved x-hat: a LayerNorm
//   writes it and nobody reads it, and no LayerNorm runs between an attention and the projection that consumes y
constexpr int kMatFwdTiles = 10;
constexpr int mat_fwd_tile(int k) {
    return k == cENC_ ? 0
         : (k >= S0_ && k <= S3_) ? 1 + (k - S0_)
         : (k == cZ1_ || k == cZM_ || k == cZH_ || k == aZ_ || k == aZM_ || k == aZH_) ? 5
         : (k == cQ_ || k == aQ1_ || k == aQ2_) ? 6
         : (k == cK_ || k == aK1_ || k == aK2_) ? 7
         : (k == cV_ || k == aV1_ || k == aV2_) ? 8
         : 9;                                                // y, x-hat; S4 / DENC exist only in the backward
}

// Observation widths: up to kMONarrow the rows are staged whole in LDS; wider ones (WIDE, up to kMOWide) stream through two
// [16][kMOCS] chunk tiles of kMOC columns (mat_obs_encoder_wide), so the carve is that of a kMONarrow-wide launch plus the
// [16] row means -- two whole [16][pad16(O) + 4] tiles beside the 34 activation tiles pass the CU's 160 KiB at O = 49.
constexpr int kMONarrow = 32, kMOWide = 128;
constexpr int kMOC = 32;           // columns of a chunk
constexpr int kMOCS = kMOC + 4;    // row stride of a chunk tile

// LDS carve shared by the update kernel (K15), the rollout step kernel (K16) and, with FWD, the evaluation step (K20)
template <bool FWD, bool WIDE = false>
struct MatCtxT {
    static constexpr bool kWide = WIDE;
    const float* P; const long* off;
    int O, L, NA, Ain, OS, n_rows;
    int* sRow; int* sAct; float* sMisc; float* sRowF; float* sRstd; float* sMean;
    float *sOutC, *sOutA, *sDOutC, *sDOutA, *sP0, *sP1, *sP2, *sS, *sXA, *sXO, *sYO, *T;
    __device__ __forceinline__ float* tile(int k) const { return T + (long)(FWD ? mat_fwd_tile(k) : k) * kMTile; }
    __device__ __forceinline__ float* rstd(int k) const { return sRstd + 16 * k; }
    __device__ __forceinline__ const float* W(int k) const { return P + off[k]; }
    __device__ __forceinline__ void carve(float* sm, int O_) {
        O = O_; OS = WIDE ? kMOCS : 16 * ((O_ + 15) >> 4) + 4;
        sRow = reinterpret_cast<int*>(sm);                 // [16] buffer row of the token's env (-1: padding)
        sAct = reinterpret_cast<int*>(sm) + 16;            // [16] action of the token
        sMisc = sm + 32;                                   // [8] adv mean/std, vn mean/var
        sRowF = sm + 48;                                   // [3][16] adv, old log-prob, rewards-to-go
        sRstd = sm + 96;                                   // [10][16]
        sOutC = sm + 256;                                  // [16][8] critic output (col 0)
        sOutA = sOutC + 128;                               // [16][8] logits
        if constexpr (FWD) {
            sDOutC = sDOutA = nullptr;
            sP0 = sP1 = sP2 = sS = sOutA + 128;            // one probability tile [16][17]: the attentions run one at a time
            sXA = sP0 + 272;                               // [16][kMXS] action tokens
            sYO = sXA + kRows * kMXS;                      // [16][OS] observations, then the observation LayerNorm's output
            sMean = sYO + kRows * OS;                      // WIDE: [16] row means
            T = sMean + (WIDE ? kRows : 0);
            sXO = tile(cY_);                               // its x-hat: unread (OS <= kMHS, so it fits the tile); WIDE: the
                                                           // second chunk tile
        } else {
            sDOutC = sOutA + 128;
            sDOutA = sDOutC + 128;
            sP0 = sDOutA + 128;                            // 3 probability tiles + 1 dS scratch, [16][17] each
            sP1 = sP0 + 272;
            sP2 = sP1 + 272;
            sS = sP2 + 272;
            sXA = sS + 272;                                // [16][kMXS] action tokens
            sXO = sXA + kRows * kMXS;                      // [16][OS] xhat of the observation LayerNorm
            sYO = sXO + kRows * OS;                        // [16][OS] its output (input of the encoder linear)
            sMean = sYO + kRows * OS;                      // WIDE (sXO / sYO are the two chunk tiles): [16] row means
            T = sMean + (WIDE ? kRows : 0);                // [16][68] tiles from here on
        }
    }
};
using MatCtx = MatCtxT<false>;

#define MAT_TILES(c)                                                                                              \
    float *cZ1 = c.tile(cZ1_), *cN0 = c.tile(cN0_), *cQ = c.tile(cQ_), *cK = c.tile(cK_), *cV = c.tile(cV_),       \
          *cY = c.tile(cY_), *cN1 = c.tile(cN1_), *cZM = c.tile(cZM_), *cN2 = c.tile(cN2_), *cENC = c.tile(cENC_), \
          *cZH = c.tile(cZH_), *cNH = c.tile(cNH_);                                                               \
    float *aZ = c.tile(aZ_), *aN0 = c.tile(aN0_), *aQ1 = c.tile(aQ1_), *aK1 = c.tile(aK1_), *aV1 = c.tile(aV1_),   \
          *aY1 = c.tile(aY1_), *aN1 = c.tile(aN1_), *aK2 = c.tile(aK2_), *aV2 = c.tile(aV2_), *aQ2 = c.tile(aQ2_), \
          *aY2 = c.tile(aY2_), *aN2 = c.tile(aN2_), *aZM = c.tile(aZM_), *aN3 = c.tile(aN3_), *aZH = c.tile(aZH_), \
          *aNH = c.tile(aNH_);                                                                                    \
    float *S0 = c.tile(S0_), *S1 = c.tile(S1_), *S2 = c.tile(S2_), *S3 = c.tile(S3_), *S4 = c.tile(S4_),           \
          *DENC = c.tile(DENC_);                                                                                  \
    (void)cZ1; (void)cN0; (void)cQ; (void)cK; (void)cV; (void)cY; (void)cN1; (void)cZM; (void)cN2; (void)cENC;     \
    (void)cZH; (void)cNH; (void)aZ; (void)aN0; (void)aQ1; (void)aK1; (void)aV1; (void)aY1; (void)aN1; (void)aK2;   \
    (void)aV2; (void)aQ2; (void)aY2; (void)aN2; (void)aZM; (void)aN3; (void)aZH; (void)aNH; (void)S0; (void)S1;   \
    (void)S2; (void)S3; (void)S4; (void)DENC;                                                                     \
    float *sXA = c.sXA, *sXO = c.sXO, *sYO = c.sYO, *sP0 = c.sP0, *sP1 = c.sP1, *sP2 = c.sP2, *sS = c.sS,          \
          *sOutC = c.sOutC, *sOutA = c.sOutA;                                                                     \
    (void)sXA; (void)sXO; (void)sYO; (void)sP0; (void)sP1; (void)sP2; (void)sS; (void)sOutC; (void)sOutA;          \
    const int O = c.O, L = c.L, NA = c.NA, Ain = c.Ain, OS = c.OS, n_rows = c.n_rows;                              \
    (void)O; (void)L; (void)NA; (void)Ain; (void)OS; (void)n_rows;                                                \
    auto W = [&](int k) -> const float* { return c.W(k); };                                                       \
    auto rstd = [&](int k) -> float* { return c.rstd(k); };                                                       \
    (void)W; (void)rstd

// split-wgrad chain: the forward publishes every linear's input tile the moment it is settled (the backward then has
// no reason to rebuild it from the saved normalised activations); K16 and the slab form publish nothing
struct MatNoPub { __device__ __forceinline__ void operator()(int, const float*) const {} };
struct MatPanelPub {
    float* xpanel; long plane; int g, tid;
    __device__ __forceinline__ void operator()(int xid, const float* T) const { publish_tile(T, xpanel + (long)xid * plane, g, tid); }
};

// obs_encoder.0 + obs_encoder.1 of a WIDE carve: LayerNorm(O) -> Linear(O, 64) pre-GELU values -> `out`, no barrier after.
// Thread (row = tid >> 4, l = tid & 15) holds columns l + 16 j of its row, read from global memory (orow: the token's
// observation row, nullptr for a padding row -- read as zeros, as the staged form's zeroed tile); mean and rstd by
// tile_ln_fwd's two-pass arithmetic, both kept for the backward.  Then per chunk of kMOC columns: y = xhat g + b into one of
// the two chunk tiles (alternating: one barrier per chunk), accumulated into the wave's MFMA chain with k ascending.
template <typename Ctx>
__device__ __forceinline__ void mat_obs_encoder_wide(const Ctx& c, const float* __restrict__ orow, float* __restrict__ out,
                                                     int tid, int wave, int lane) {
    const int O = c.O, row = tid >> 4, l = tid & 15;
    const float* __restrict__ g = c.W(C_OLN_G);
    const float* __restrict__ b = c.W(C_OLN_B);
    constexpr int NJ = kMOWide / 16;
    float x[NJ], s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int col = l + 16 * j; x[j] = (orow && col < O) ? orow[col] : 0.f; s += x[j]; }
    const float mean = group16_sum(s) / (float)O;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int col = l + 16 * j; x[j] = col < O ? x[j] - mean : 0.f; q += x[j] * x[j]; }
    const float rs = 1.0f / sqrtf(group16_sum(q) / (float)O + 1e-5f);
    if (l == 0) { c.rstd(0)[row] = rs; c.sMean[row] = mean; }
    const float bv = c.W(C_ENC_B)[wave * 16 + (lane & 15)];
    f32x4 acc = {bv, bv, bv, bv};
#pragma unroll
    for (int ci = 0; ci < kMOWide / kMOC; ++ci) {
        const int c0 = kMOC * ci;
        if (c0 < O) {                                                  // uniform: every thread meets the barrier
            float* Y = (ci & 1) ? c.sXO : c.sYO;
#pragma unroll
            for (int jj = 0; jj < kMOC / 16; ++jj) {
                const int col = c0 + l + 16 * jj;
                Y[row * kMOCS + l + 16 * jj] = col < O ? x[(kMOC / 16) * ci + jj] * rs * g[col] + b[col] : 0.f;
            }
            MAT_SYNC();
            const int cw = O - c0 < kMOC ? O - c0 : kMOC;
            narrow_fwd_acc(c.W(C_ENC_W), O, c0, 16 * ((cw + 15) >> 4), Y, kMOCS, acc, wave, lane);
        }
    }
    narrow_store(acc, out, wave, lane);
}

// critic (encoder): observations in sYO (a WIDE carve: read through orow) -> rep_enc in cENC, value in sOutC[:, 0]; ends
// WITHOUT a barrier
// PF (K15): the fragments of linear `n` are requested one phase ahead -- MAT_NEXT(n) at the start of the phase before;
// else (K16: its registers are spoken for) at the point of use
#define MAT_LIN(r, Wk, Bk, A, out) do { if (!PF) pf_fwd(W(Wk), W(Bk), wave, lane, r); lin_fwd_r(r, A, out, wave, lane); } while (0)
#define MAT_NEXT(r, Wk, Bk) do { if (PF) pf_fwd(W(Wk), W(Bk), wave, lane, r); } while (0)
// VALUE = false (K20): stops at rep_enc, after a barrier -- the three phases of the value head are not run
template <bool PF, typename Pub = MatNoPub, bool VALUE = true, typename Ctx = MatCtx>
__device__ __forceinline__ void mat_encoder_forward(const Ctx& c, int tid, int wave, int lane, const Pub pub = Pub(),
                                                    const float* orow = nullptr) {
    MAT_TILES(c);
    MatFr rq, rk, rv, rp, rm1, rm2, rh1;
    MAT_NEXT(rq, C_Q_W, C_Q_B); MAT_NEXT(rk, C_K_W, C_K_B); MAT_NEXT(rv, C_V_W, C_V_B);       // two phases ahead of their use
    if constexpr (Ctx::kWide) {
        mat_obs_encoder_wide(c, orow, cZ1, tid, wave, lane);                                  // obs_encoder.0 and .1
    } else {
        tile_ln_fwd(sYO, OS, O, W(C_OLN_G), W(C_OLN_B), sXO, rstd(0), sYO, tid);              // obs_encoder.0
        MAT_SYNC();
        MAT_STAMP(16);
        narrow_fwd(W(C_ENC_W), O, W(C_ENC_B), sYO, OS, cZ1, wave, lane);                      // obs_encoder.1
    }
    MAT_SYNC();
    MAT_STAMP(17);
    tile_gelu(cZ1, S0, tid);
    tile_ln_fwd(S0, kMHS, kMD, W(C_LN_G), W(C_LN_B), cN0, rstd(1), S1, tid);                  // critic.ln -> H0 in S1
    MAT_SYNC();
    MAT_STAMP(18);
    pub(X_H0, S1);
    MAT_NEXT(rp, C_P_W, C_P_B);
    MAT_LIN(rq, C_Q_W, C_Q_B, S1, cQ);
    MAT_LIN(rk, C_K_W, C_K_B, S1, cK);
    MAT_LIN(rv, C_V_W, C_V_B, S1, cV);
    MAT_SYNC();
    MAT_STAMP(19);
    att_fwd(cQ, cK, cV, cY, sP0, L, n_rows, false, wave, lane);
    MAT_SYNC();
    MAT_STAMP(20);
    pub(X_CY, cY);
    MAT_NEXT(rm1, C_M1_W, C_M1_B);
    MAT_LIN(rp, C_P_W, C_P_B, cY, S2);
    MAT_SYNC();
    MAT_STAMP(21);
    tile_add(S1, S2, S2, tid);
    tile_ln_fwd(S2, kMHS, kMD, W(C_LN1_G), W(C_LN1_B), cN1, rstd(2), S0, tid);                // H1 in S0
    MAT_SYNC();
    MAT_STAMP(22);
    pub(X_H1, S0);
    MAT_NEXT(rm2, C_M2_W, C_M2_B);
    MAT_LIN(rm1, C_M1_W, C_M1_B, S0, cZM);
    MAT_SYNC();
    MAT_STAMP(23);
    tile_gelu(cZM, S2, tid);
    MAT_SYNC();
    MAT_STAMP(24);
    pub(X_GCM, S2);
    MAT_NEXT(rh1, C_H1_W, C_H1_B);
    MAT_LIN(rm2, C_M2_W, C_M2_B, S2, S3);
    MAT_SYNC();
    MAT_STAMP(25);
    tile_add(S0, S3, S3, tid);
    tile_ln_fwd(S3, kMHS, kMD, W(C_LN2_G), W(C_LN2_B), cN2, rstd(3), cENC, tid);              // rep_enc
    MAT_SYNC();
    MAT_STAMP(26);
    pub(X_ENC, cENC);
    if constexpr (!VALUE) return;
    MAT_LIN(rh1, C_H1_W, C_H1_B, cENC, cZH);
    MAT_SYNC();
    MAT_STAMP(27);
    tile_gelu(cZH, S0, tid);
    tile_ln_fwd(S0, kMHS, kMD, W(C_HLN_G), W(C_HLN_B), cNH, rstd(4), S1, tid);
    MAT_SYNC();
    MAT_STAMP(28);
    head_out_fwd(W(C_H2_W), W(C_H2_B), 1, S1, sOutC, tid);

}

// actor (decoder): token block in sXA + rep_enc in cENC -> logits in sOutA; starts and ends with the tiles settled
template <bool PF, typename Pub = MatNoPub, typename Ctx = MatCtx>
__device__ __forceinline__ void mat_decoder_forward(const Ctx& c, int tid, int wave, int lane, const Pub pub = Pub(),
                                                    const float* enc_bias = nullptr) {
    MAT_TILES(c);
    MatFr rk1, rq1, rv1, rp1, rk2, rv2, rq2, rp2, rm1, rm2, rh1;
    MAT_NEXT(rk1, A_K1_W, A_K1_B); MAT_NEXT(rq1, A_Q1_W, A_Q1_B); MAT_NEXT(rv1, A_V1_W, A_V1_B);
    narrow_fwd(W(A_ENC_W), Ain, enc_bias, sXA, kMXS, aZ, wave, lane);                         // action_encoder.0 (Box: a bias)
    MAT_SYNC();
    tile_gelu(aZ, S0, tid);
    tile_ln_fwd(S0, kMHS, kMD, W(A_LN_G), W(A_LN_B), aN0, rstd(5), S1, tid);                  // x0 in S1
    MAT_SYNC();
    pub(X_X0, S1);
    MAT_NEXT(rp1, A_P1_W, A_P1_B);
    MAT_LIN(rk1, A_K1_W, A_K1_B, S1, aK1);
    MAT_LIN(rq1, A_Q1_W, A_Q1_B, S1, aQ1);
    MAT_LIN(rv1, A_V1_W, A_V1_B, S1, aV1);
    MAT_SYNC();
    att_fwd(aQ1, aK1, aV1, aY1, sP1, L, n_rows, true, wave, lane);
    MAT_SYNC();
    pub(X_AY1, aY1);
    MAT_NEXT(rk2, A_K2_W, A_K2_B); MAT_NEXT(rv2, A_V2_W, A_V2_B); MAT_NEXT(rq2, A_Q2_W, A_Q2_B);
    MAT_LIN(rp1, A_P1_W, A_P1_B, aY1, S2);
    MAT_SYNC();
    tile_add(S1, S2, S2, tid);
    tile_ln_fwd(S2, kMHS, kMD, W(A_LN1_G), W(A_LN1_B), aN1, rstd(6), S0, tid);                // x1 in S0
    MAT_SYNC();
    pub(X_X1, S0);
    MAT_NEXT(rp2, A_P2_W, A_P2_B);
    MAT_LIN(rk2, A_K2_W, A_K2_B, S0, aK2);                                       // key = value = x1
    MAT_LIN(rv2, A_V2_W, A_V2_B, S0, aV2);
    MAT_LIN(rq2, A_Q2_W, A_Q2_B, cENC, aQ2);                                     // query = rep_enc
    MAT_SYNC();
    att_fwd(aQ2, aK2, aV2, aY2, sP2, L, n_rows, true, wave, lane);
    MAT_SYNC();
    pub(X_AY2, aY2);
    MAT_NEXT(rm1, A_M1_W, A_M1_B);
    MAT_LIN(rp2, A_P2_W, A_P2_B, aY2, S2);
    MAT_SYNC();
    tile_add(cENC, S2, S2, tid);
    tile_ln_fwd(S2, kMHS, kMD, W(A_LN2_G), W(A_LN2_B), aN2, rstd(7), S1, tid);                // x2 in S1
    MAT_SYNC();
    pub(X_X2, S1);
    MAT_NEXT(rm2, A_M2_W, A_M2_B);
    MAT_LIN(rm1, A_M1_W, A_M1_B, S1, aZM);
    MAT_SYNC();
    tile_gelu(aZM, S2, tid);
    MAT_SYNC();
    pub(X_GAM, S2);
    MAT_NEXT(rh1, A_H1_W, A_H1_B);
    MAT_LIN(rm2, A_M2_W, A_M2_B, S2, S3);
    MAT_SYNC();
    tile_add(S1, S3, S3, tid);
    tile_ln_fwd(S3, kMHS, kMD, W(A_LN3_G), W(A_LN3_B), aN3, rstd(8), S0, tid);                // x3 in S0
    MAT_SYNC();
    pub(X_X3, S0);
    MAT_LIN(rh1, A_H1_W, A_H1_B, S0, aZH);
    MAT_SYNC();
    tile_gelu(aZH, S2, tid);
    tile_ln_fwd(S2, kMHS, kMD, W(A_HLN_G), W(A_HLN_B), aNH, rstd(9), S1, tid);                // head LayerNorm output in S1
    MAT_SYNC();
    head_out_fwd(W(A_H2_W), W(A_H2_B), NA, S1, sOutA, tid);
    MAT_SYNC();

}

}  // namespace ppoaf
