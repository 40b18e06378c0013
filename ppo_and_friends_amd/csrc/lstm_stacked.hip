// K18 for two stacked LSTM layers: LSTMNetwork(num_lstm_layers=2).forward_logits -- forward, backward through the head
// and time, weight gradients.  The one-layer kernels (lstm.hip) and their bodies (lstm_device.hpp) are untouched; this
// file includes their helpers.
//
// Forward: one workgroup per tile of 16 rows, 2 H / 16 waves.  Waves [0, H/16) own layer 0, waves [H/16, 2H/16) layer 1,
// each wave the hidden slice [16 w, 16 w + 16) of all four gates of its layer, so a lane holds i, f, g, o of the same
// (row, unit) pairs and its cell state stays in registers.  The two recurrences run as a wavefront: in phase p
// (0 <= p <= S) layer 0 computes step p and layer 1 step p - 1,
//
//      phase      0        1        2       ...      S-1        S
//      layer 0   t=0      t=1      t=2      ...     t=S-1       --
//      layer 1    --      t=0      t=1      ...     t=S-2      t=S-1
//
// with ONE barrier per phase: S + 1 barriers for 2 S cell updates.  Layer 1's input h0_{p-1} is the very LDS tile that
// layer 0 reads as its recurrent operand in the same phase, so it is staged once.  LDS: x double-buffered, h of layer 0
// and h of layer 1 double-buffered (h_t of a layer lies in buffer (t + 1) & 1, the initial state in buffer 0); the
// head's buffers reuse the x buffers once phase S has passed.  H = 32: every wave keeps its gate blocks in VGPRs for
// the window (layer 0 W_hh, layer 1 W_ih and W_hh); H = 64: W_hh of the wave's layer resident, layer 1 streams W_ih a gate
// block at a time; H = 128 re-reads both every step, half a gate block at a time.
//
// Backward: H / 16 waves, the layers in turn.  Head and LayerNorm as the one-layer body, then layer 1 backwards over the
// steps -- its gate gradients go through LDS, the MFMA forms d h1_{t-1} (W_hh_l1^T, resident) and the part of d h0_t that
// comes through W_ih_l1^T, which is left in the workspace per (row, step) -- then layer 0 over the steps with
// d h0_t = (workspace) + (its own step t + 1).  The lane that wrote an element of d h0_t is the lane that reads it.
// Every sum has one fixed order.  The weight gradients are lstm_wgrad_tile<true> over a job table of this file's own size.
#include "lstm_stacked_device.hpp"

namespace ppoaf {
namespace {

constexpr int kL2MaxJobs = 16;

template <int H>
__global__ __launch_bounds__(2 * (H / 16) * 64) PPOAF_NO_PK_F32 void lstm2_forward_kernel(const Lstm2Args a) {
    constexpr int HT = H / 16, NW = 2 * HT, NT = NW * 64, HS = H + 4, XS = kLMaxIn + 4;
    static_assert(2 * kLRows * XS >= kLRows * HS + 2 * kLRows * kLFS, "head buffers reuse the x buffers");
    __shared__ float xs[2 * kLRows * XS];
    __shared__ float h0s[2][kLRows * HS];
    __shared__ float h1s[2][kLRows * HS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the layer branches below are whole-wave branches
    const bool upper = w >= HT;                               // wave-uniform: this wave works on layer 1
    const int wl = upper ? w - HT : w;
    const long r0 = (long)blockIdx.x * kLRows;
    const long N = a.N;
    const int S = a.S, I = a.I, Ip = (a.I + 15) & ~15;
    const int j = 16 * wl + (lane & 15);
    const float* Wih0 = a.P + a.L.w_ih[0];
    const float* Wih1 = a.P + a.L.w_ih[1];
    // (both layers' offsets are read and one is picked by arithmetic: a select between two loads of the argument struct
    //  becomes a load at a computed address, which moves the whole struct to the private segment)
    const long up = upper ? 1 : 0;
    const float* Whh = a.P + (a.L.w_hh[0] + up * (a.L.w_hh[1] - a.L.w_hh[0]));
    const long lofs = up * a.ls;
    const long wgates = a.L.gates[0] + up * (a.L.gates[1] - a.L.gates[0]), wcst = a.L.cst[0] + up * (a.L.cst[1] - a.L.cst[0]);
    const long whst = a.L.hst[0] + up * (a.L.hst[1] - a.L.hst[0]);

    // Resident gate blocks: H = 32 -- layer 0: fr[q] = W_hh_l0 of gate q; layer 1: fr[q] = W_hh_l1, fr[4 + q] = W_ih_l1.
    // H = 64 -- fr[q] = W_hh of the wave's layer; layer 1 streams W_ih_l1, a gate block (16 registers) in flight (both
    // matrices resident left no room for the cell update: 42 registers went to the private segment).  H = 128 (16 waves:
    // 128 registers per lane) -- nothing resident, half a gate block (16 rows x 64 columns) in flight, from the L1 / L2.
    constexpr bool kResident = H <= 64;
    constexpr int KC = H == 128 ? HT / 2 : HT;                // chunks of a streamed gate block in flight
    float4 fr[H == 32 ? 8 : kResident ? 4 : 1][kResident ? HT : 1];
    const __amdgpu_buffer_rsrc_t rsI = frag_rsrc(Wih1), rsH = frag_rsrc(Whh);
    const unsigned foff = (unsigned)(((16 * wl + (lane & 15)) * H + 4 * (lane >> 4)) * 4);
    const __amdgpu_buffer_rsrc_t rs0 = frag_rsrc(Wih0);
    const unsigned xoff = (unsigned)((j * I + 4 * (lane >> 4)) * 4);
    auto wih0 = [&](const int disp) __attribute__((always_inline)) {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs0, xoff, disp, 0));
    };
    // init + A (16 rows x H, LDS) x (gate q's rows [16 wl, 16 wl + 16) of the [4H, H] matrix behind rs)^T
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
                __builtin_amdgcn_sched_barrier(0);            // (one half in flight: the scheduler would hoist every unrolled load)
                load_fwd_frags_rs<KC>(rs, foff, (q * H * H + 16 * KC * hh) * 4, ft);
                acc = acc + mfma_rows_x_frags<KC>(A + 16 * KC * hh, HS, lane, ft, 0.f);
            }
            return acc;
        }
    };
    if constexpr (kResident) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            load_fwd_frags<HT>(Whh, q * H + 16 * wl, lane, fr[q]);
            if constexpr (H == 32) {
                if (upper) load_fwd_frags<HT>(Wih1, q * H + 16 * wl, lane, fr[4 + q]);
            }
        }
    }
    float bias[4];
    {
        const long bi = a.L.b_ih[0] + up * (a.L.b_ih[1] - a.L.b_ih[0]), bh = a.L.b_hh[0] + up * (a.L.b_hh[1] - a.L.b_hh[0]);
#pragma unroll
        for (int q = 0; q < 4; ++q) bias[q] = a.P[bi + q * H + j] + a.P[bh + q * H + j];
    }

    auto load_x = [&](int t, float* dst) __attribute__((always_inline)) {      // (a call would keep `a` in the private segment)
        for (int e = tid; e < kLRows * Ip; e += NT) {
            const int r = e / Ip, k = e - r * Ip;
            const long n = r0 + r;
            dst[r * XS + k] = (n < N && k < I) ? a.x[(n * S + t) * I + k] : 0.f;
        }
    };
    for (int e = tid; e < kLRows * H; e += NT) {
        const int r = e / H, k = e - r * H;
        const long n = r0 + r;
        const float v0 = n < N ? a.h0[n * a.rs + k] : 0.f;
        const float v1 = n < N ? a.h0[n * a.rs + a.ls + k] : 0.f;
        h0s[0][r * HS + k] = v0;
        h1s[0][r * HS + k] = v1;
        if (a.stash && n < N) { a.ws[a.L.hinit[0] + n * H + k] = v0; a.ws[a.L.hinit[1] + n * H + k] = v1; }
    }
    float cr[4], hr[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long n = r0 + 4 * (lane >> 4) + g;
        cr[g] = n < N ? a.c0[n * a.rs + lofs + j] : 0.f;
        hr[g] = n < N ? a.h0[n * a.rs + lofs + j] : 0.f;
    }
    load_x(0, xs);
    __syncthreads();

    for (int p = 0; p <= S; ++p) {
        const float* h0b = h0s[p & 1];                        // h0_{p-1}: layer 0's recurrent operand, layer 1's input
        const int t = p - (int)up;                            // this wave's step in phase p; one cell update for both layers
        f32x4 z[4];
        if (t >= 0 && t < S) {
            if (!upper) {
                const float* xb = xs + (p & 1) * kLRows * XS;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 acc = {bias[q], bias[q], bias[q], bias[q]};
#pragma unroll 1
                    for (int c = 0; c < Ip / 16; ++c) {
                        const int k0 = 16 * c + 4 * (lane >> 4);
                        const float4 x4 = *reinterpret_cast<const float4*>(xb + (lane & 15) * XS + k0);
                        const int wd = (q * H * I + 16 * c) * 4;          // row q H + j of W_ih_l0, columns from 16 c: one lane offset
                        const float b0 = k0 < I ? wih0(wd) : 0.f, b1 = k0 + 1 < I ? wih0(wd + 4) : 0.f;
                        const float b2 = k0 + 2 < I ? wih0(wd + 8) : 0.f, b3 = k0 + 3 < I ? wih0(wd + 12) : 0.f;
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.x, b0, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.y, b1, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.z, b2, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.w, b3, acc, 0, 0, 0);
                    }
                    if constexpr (kResident) z[q] = acc + mfma_rows_x_frags<HT>(h0b, HS, lane, fr[q], 0.f);
                    else z[q] = acc + streamed(rsH, q, h0b, 0.f);
                }
            } else {
                const float* h1b = h1s[(p - 1) & 1];          // h1_{p-2}
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 acc;
                    if constexpr (H == 32) acc = mfma_rows_x_frags<HT>(h0b, HS, lane, fr[4 + q], bias[q]);
                    else acc = streamed(rsI, q, h0b, bias[q]);
                    if constexpr (kResident) z[q] = acc + mfma_rows_x_frags<HT>(h1b, HS, lane, fr[q], 0.f);
                    else z[q] = acc + streamed(rsH, q, h1b, 0.f);
                }
            }
            lstm2_cell<H>(a, z, cr, hr, upper ? h1s[p & 1] : h0s[(p + 1) & 1], wgates, wcst, whst, r0, t, j, lane);
        }
        if (p + 1 < S) load_x(p + 1, xs + ((p + 1) & 1) * kLRows * XS);
        __syncthreads();
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long n = r0 + 4 * (lane >> 4) + g;
        if (n < N) {
            if (a.hn) a.hn[n * a.rs + lofs + j] = hr[g];
            if (a.cn) a.cn[n * a.rs + lofs + j] = cr[g];
        }
    }
    const float* hfin = h1s[S & 1];

    // ---- head: LayerNorm(H) -> activation -> Linear layers on all 2 H / 16 waves (the x buffers are free now); every
    //      element's arithmetic is the one-layer body's
    float* A0 = xs;
    float* A1 = xs + kLRows * HS;
    float* A2 = A1 + kLRows * kLFS;
    for (int r = w; r < kLRows; r += NW) {
        const long n = r0 + r;
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s += hfin[r * HS + k];
        const float mean = wave_sum(s) / (float)H;
        float v = 0.f;
        for (int k = lane; k < H; k += 64) { const float d = hfin[r * HS + k] - mean; v += d * d; }
        const float rstd = 1.f / sqrtf(wave_sum(v) / (float)H + 1e-5f);
        for (int k = lane; k < H; k += 64) {
            const float y = (hfin[r * HS + k] - mean) * rstd * a.P[a.L.ln_w + k] + a.P[a.L.ln_b + k];
            const float y2 = act_fwd(y, a.act);
            A0[r * HS + k] = y2;
            if (a.stash && n < N) a.ws[a.L.acts[0] + n * H + k] = y2;
        }
        if (a.stash && n < N && lane == 0) { a.ws[a.L.stats + 2 * n] = mean; a.ws[a.L.stats + 2 * n + 1] = rstd; }
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
        const long acts = l == 0 ? a.L.acts[1] : a.L.acts[2];
        for (int e = tid; e < kLRows * M; e += NT) {
            const int r = e / M, m = e - r * M;
            const long n = r0 + r;
            const float* ir = in + r * IS;
            const float* wr = W + (long)m * K;
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += ir[k] * wr[k];
            s += b[m];
            if (last) {
                if (n < N) a.out[n * M + m] = s;
            } else {
                s = act_fwd(s, a.act);
                ob[r * kLFS + m] = s;
                if (a.stash && n < N) a.ws[acts + n * M + m] = s;
            }
        }
        __syncthreads();
        in = ob; IS = kLFS; K = M;
    }
}

// One step of the backward recurrence of a layer for this lane's four (row, unit) pairs: d h_t (dh) and the cell
// gradient carried from step t + 1 (dc) -> the pre-activation gate gradients, to the workspace plane `dG` and to the LDS
// plane `gb` (zeros for dead rows); dc becomes the carry into step t - 1.
template <int H>
__device__ __forceinline__ void lstm2_gate_grads(const Lstm2Args& a, const float (&dh)[4], float (&dc)[4], float* gb,
                                                 const long gates, const long cst, const long dG, const float* c0,
                                                 const long r0, const int t, const int j, const int lane) {
    constexpr int GS = 4 * H + 4;
    const int S = a.S;
    float* ws = a.ws;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int rr = 4 * (lane >> 4) + g;
        const long n = r0 + rr;
        float dai = 0.f, daf = 0.f, dag = 0.f, dao = 0.f;
        if (n < a.N) {
            const float* gp = ws + gates + (n * S + t) * 4 * H + j;
            const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
            const float ct = ws[cst + (n * S + t) * H + j];
            const float cp = t > 0 ? ws[cst + (n * S + t - 1) * H + j] : c0[n * a.rs + j];
            const float tc = tanhf(ct);
            const float dcv = dc[g] + dh[g] * og * (1.f - tc * tc);
            dai = dcv * gg * (ig * (1.f - ig));
            daf = dcv * cp * (fg * (1.f - fg));
            dag = dcv * ig * (1.f - gg * gg);
            dao = dh[g] * tc * (og * (1.f - og));
            dc[g] = dcv * fg;
            float* dp = ws + dG + (n * S + t) * 4 * H + j;
            dp[0] = dai; dp[H] = daf; dp[2 * H] = dag; dp[3 * H] = dao;
        }
        gb[rr * GS + j] = dai; gb[rr * GS + H + j] = daf; gb[rr * GS + 2 * H + j] = dag; gb[rr * GS + 3 * H + j] = dao;
    }
}

// this wave's slice of W^T for a [4H, H] matrix: B[k][col] = W[k][16 w + col], k over the 4H gate rows
template <int H>
__device__ __forceinline__ void load_wt_slice(const float* W, const int j, const int lane, float4 (&fr)[4 * (H / 16)]) {
    const float* w0 = W + (long)(4 * (lane >> 4)) * H + j;
#pragma unroll
    for (int c = 0; c < 4 * (H / 16); ++c) {
        const float* wp = w0 + (long)(16 * c) * H;
        fr[c] = make_float4(wp[0], wp[H], wp[2 * H], wp[3 * H]);
    }
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) PPOAF_NO_PK_F32 void lstm2_backward_kernel(const Lstm2Args a) {
    constexpr int HT = H / 16, NT = HT * 64, HS = H + 4, GS = 4 * H + 4;
    constexpr int kLds = 2 * kLRows * GS > 2 * kLRows * kLFS + kLRows * HS ? 2 * kLRows * GS : 2 * kLRows * kLFS + kLRows * HS;
    __shared__ float lds[kLds];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = (long)blockIdx.x * kLRows;
    const long N = a.N;
    const int S = a.S, F = a.F, D = a.D, O = a.O;
    const int j = 16 * w + (lane & 15);
    float* ws = a.ws;

    // ---- head: d logits -> d pre-activation of every Linear -> d LayerNorm output -> d h1_S (the one-layer body's sums)
    float* Bc = lds;
    float* Bn = lds + kLRows * kLFS;
    float* DH = lds + 2 * kLRows * kLFS;
    {
        const long dzD = D == 1 ? a.L.dz[1] : a.L.dz[2];
        for (int e = tid; e < kLRows * O; e += NT) {
            const int r = e / O, o = e - r * O;
            const long n = r0 + r;
            const float v = n < N ? a.dout[n * O + o] : 0.f;
            Bc[r * kLFS + o] = v;
            if (n < N) ws[dzD + n * O + o] = v;
        }
    }
    __syncthreads();
    for (int l = D; l >= 0; --l) {
        const int M = l == D ? O : F, K = l == 0 ? H : F;
        const float* W = a.P + (l == 0 ? a.L.fw[0] : l == 1 ? a.L.fw[1] : a.L.fw[2]);
        const long acts = l == 0 ? a.L.acts[0] : l == 1 ? a.L.acts[1] : a.L.acts[2];
        const long dzp = l == 2 ? a.L.dz[1] : a.L.dz[0];
        for (int e = tid; e < kLRows * K; e += NT) {
            const int r = e / K, k = e - r * K;
            const long n = r0 + r;
            float s = 0.f;
            for (int m = 0; m < M; ++m) s += Bc[r * kLFS + m] * W[(long)m * K + k];
            const float av = n < N ? ws[acts + n * K + k] : 0.f;
            const float g = n < N ? s * act_bwd(av, a.act) : 0.f;
            if (l > 0) {
                Bn[r * kLFS + k] = g;
                if (n < N) ws[dzp + n * F + k] = g;
            } else {
                DH[r * HS + k] = g;
                if (n < N) ws[a.L.dy + n * H + k] = g;
            }
        }
        __syncthreads();
        float* t = Bc; Bc = Bn; Bn = t;
    }
    for (int r = w; r < kLRows; r += HT) {
        const long n = r0 + r;
        if (n >= N) {
            for (int k = lane; k < H; k += 64) DH[r * HS + k] = 0.f;
            continue;
        }
        const float mean = ws[a.L.stats + 2 * n], rstd = ws[a.L.stats + 2 * n + 1];
        const float* hS = ws + a.L.hst[1] + (n * S + S - 1) * H;
        float xh[2] = {0.f, 0.f}, gy[2] = {0.f, 0.f};
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = lane + 64 * u;
            if (k < H) {
                xh[u] = (hS[k] - mean) * rstd;
                gy[u] = DH[r * HS + k] * a.P[a.L.ln_w + k];
                s1 += gy[u];
                s2 += gy[u] * xh[u];
                ws[a.L.xhat + n * H + k] = xh[u];
            }
        }
        s1 = wave_sum(s1) / (float)H;
        s2 = wave_sum(s2) / (float)H;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = lane + 64 * u;
            if (k < H) DH[r * HS + k] = rstd * (gy[u] - s1 - xh[u] * s2);
        }
    }
    __syncthreads();
    float dh[4], dc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { dh[g] = DH[(4 * (lane >> 4) + g) * HS + j]; dc[g] = 0.f; }

    // ---- layer 1 over t = S-1 .. 0: W_hh_l1^T resident; W_ih_l1^T resident at H <= 64, else one gate's rows at a time
    constexpr bool kResident = H <= 64;
    const float* Wih1 = a.P + a.L.w_ih[1];
    float4 frH[4 * HT];
    constexpr int HQ = kResident ? HT : HT / 4;               // H = 128: a quarter of a gate's rows in flight
    float4 frI[kResident ? 4 : 1][HQ];
    const __amdgpu_buffer_rsrc_t rsI = frag_rsrc(Wih1);
    const unsigned doff = (unsigned)((4 * (lane >> 4) * H + j) * 4);
    load_wt_slice<H>(a.P + a.L.w_hh[1], j, lane, frH);
    if constexpr (kResident) {
#pragma unroll
        for (int q = 0; q < 4; ++q) load_dgrad_frags<HT>(Wih1 + (long)q * H * H, 16 * w, lane, frI[q]);
    }
    __syncthreads();                                          // DH shares the LDS with the gate-gradient planes
    for (int t = S - 1; t >= 0; --t) {
        float* gb = lds + (t & 1) * kLRows * GS;
        lstm2_gate_grads<H>(a, dh, dc, gb, a.L.gates[1], a.L.cst[1], a.L.dG[1], a.c0 + a.ls, r0, t, j, lane);
        __syncthreads();
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (kResident) {
                d0 = d0 + mfma_rows_x_frags<HT>(gb + q * H, GS, lane, frI[q], 0.f);
            } else {
#pragma unroll
                for (int u = 0; u < HT / HQ; ++u) {
                    const int k0 = q * H + 16 * HQ * u;       // gate rows [k0, k0 + 16 HQ)
                    __builtin_amdgcn_sched_barrier(0);        // (one quarter in flight: the scheduler would hoist every unrolled load)
                    load_dgrad_frags_rs<HQ>(rsI, doff, k0, H * 4, frI[0]);
                    d0 = d0 + mfma_rows_x_frags<HQ>(gb + k0, GS, lane, frI[0], 0.f);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const long n = r0 + 4 * (lane >> 4) + g;
            if (n < N) ws[a.L.dh0 + (n * S + t) * H + j] = d0[g];
        }
        if (t > 0) {
            const f32x4 acc = mfma_rows_x_frags<4 * HT>(gb, GS, lane, frH, 0.f);
#pragma unroll
            for (int g = 0; g < 4; ++g) dh[g] = acc[g];
        }
    }

    // ---- layer 0 over t = S-1 .. 0: d h0_t = (through W_ih_l1, from the workspace: this lane's own stores) + (step t + 1)
    __syncthreads();                                          // the last plane of layer 1 has been read by every wave
    load_wt_slice<H>(a.P + a.L.w_hh[0], j, lane, frH);
    float rec[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { rec[g] = 0.f; dc[g] = 0.f; }
    for (int t = S - 1; t >= 0; --t) {
        float* gb = lds + (t & 1) * kLRows * GS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const long n = r0 + 4 * (lane >> 4) + g;
            dh[g] = (n < N ? ws[a.L.dh0 + (n * S + t) * H + j] : 0.f) + rec[g];
        }
        lstm2_gate_grads<H>(a, dh, dc, gb, a.L.gates[0], a.L.cst[0], a.L.dG[0], a.c0, r0, t, j, lane);
        __syncthreads();
        if (t > 0) {
            const f32x4 acc = mfma_rows_x_frags<4 * HT>(gb, GS, lane, frH, 0.f);
#pragma unroll
            for (int g = 0; g < 4; ++g) rec[g] = acc[g];
        }
    }
}

struct WJobs2 {
    WJob j[kL2MaxJobs];
    int n;
};

__global__ __launch_bounds__(256) PPOAF_NO_PK_F32 void lstm2_wgrad_kernel(const WJobs2 J) {
    __shared__ float part[4][64][4];
    int ji = 0;
    while (ji + 1 < J.n && (int)blockIdx.x >= J.j[ji + 1].tile_begin) ++ji;
    lstm_wgrad_tile<true>(J.j[ji], blockIdx.x - J.j[ji].tile_begin, part);
}

// host: every weight-gradient job of the two-layer network; returns the tile count
int lstm2_wgrad_jobs(WJobs2& J, const Lstm2Args& a, const int H, const float* x, float* G) {
    const Lstm2Layout& L = a.L;
    const long N = a.N, S = a.S, NS = N * S;
    const int I = a.I, F = a.F, D = a.D, O = a.O;
    const float* ws = a.ws;
    int nt = 0;
    auto add = [&](const float* A, int lda, const float* B, int ldb, const float* B0, int M, int Nc, int mode,
                   long K, float* out, float* out2, int ldo) {
        WJob& jb = J.j[J.n++];
        jb.A = A; jb.lda = lda; jb.B = B; jb.ldb = ldb; jb.B0 = B0; jb.M = M; jb.Nc = Nc; jb.mode = mode;
        jb.K = K; jb.out = out; jb.out2 = out2; jb.ldo = ldo; jb.S = (int)S;
        jb.tiles_n = (Nc + 15) / 16;
        jb.tile_begin = nt;
        nt += (mode == kBDiag ? 1 : (M + 15) / 16) * jb.tiles_n;
    };
    for (int l = 0; l < 2; ++l) {
        const float* dG = ws + L.dG[l];
        if (l == 0) add(dG, 4 * H, x, I, nullptr, 4 * H, I, kBDense, NS, G + L.w_ih[0], nullptr, I);
        else add(dG, 4 * H, ws + L.hst[0], H, nullptr, 4 * H, H, kBDense, NS, G + L.w_ih[1], nullptr, H);   // the input is h0_t
        add(dG, 4 * H, ws + L.hst[l], H, ws + L.hinit[l], 4 * H, H, kBHPrev, NS, G + L.w_hh[l], nullptr, H);
        add(dG, 4 * H, nullptr, 0, nullptr, 4 * H, 1, kBOnes, NS, G + L.b_ih[l], G + L.b_hh[l], 1);
    }
    add(ws + L.dy, H, ws + L.xhat, H, nullptr, 1, H, kBDiag, N, G + L.ln_w, nullptr, 1);
    add(ws + L.dy, H, nullptr, H, nullptr, 1, H, kBDiag, N, G + L.ln_b, nullptr, 1);
    for (int l = 0; l <= D; ++l) {
        const int M = l == D ? O : F, K = l == 0 ? H : F;
        add(ws + L.dz[l], M, ws + L.acts[l], K, nullptr, M, K, kBDense, N, G + L.fw[l], nullptr, K);
        add(ws + L.dz[l], M, nullptr, 0, nullptr, M, 1, kBOnes, N, G + L.fb[l], nullptr, 1);
    }
    return nt;
}

template <int H>
int launch_forward(const Lstm2Args& a, hipStream_t s) {
    const unsigned blocks = (unsigned)((a.N + kLRows - 1) / kLRows);
    hipLaunchKernelGGL(lstm2_forward_kernel<H>, dim3(blocks), dim3(2 * (H / 16) * 64), 0, s, a);
    return check_launch("ppoaf_lstm2_forward");
}

template <int H>
int launch_backward(const Lstm2Args& a, hipStream_t s) {
    const unsigned blocks = (unsigned)((a.N + kLRows - 1) / kLRows);
    hipLaunchKernelGGL(lstm2_backward_kernel<H>, dim3(blocks), dim3(H / 16 * 64), 0, s, a);
    return check_launch("ppoaf_lstm2_backward");
}

}  // namespace
}  // namespace ppoaf

using namespace ppoaf;

#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, in_dim, 0);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, hidden, 4);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, ff_hidden, 8);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, ff_depth, 12);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, out_dim, 16);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, activation, 20);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, rows, 24);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, steps, 32);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, params, 40);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, grads, 48);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, workspace, 56);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, workspace_floats, 64);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, state_row_stride, 72);
PPOAF_LAYOUT(ppoaf_lstm2_desc_t, state_layer_stride, 80);
static_assert(sizeof(ppoaf_lstm2_desc_t) == 88, "ppoaf_lstm2_desc_t");
static_assert(sizeof(ppoaf_lstm_desc_t) == 72, "ppoaf_lstm_desc_t keeps its size");

extern "C" int ppoaf_lstm2_check(const ppoaf_lstm2_desc_t* d, int32_t need_workspace) {
    return check_lstm2_desc(d, need_workspace != 0, "ppoaf_lstm2_check");
}

extern "C" int ppoaf_lstm2_workspace_floats(const ppoaf_lstm2_desc_t* d, int64_t* floats_out) {
    if (int rc = check_lstm2_desc(d, false, "ppoaf_lstm2_workspace_floats")) return rc;
    PPOAF_REQUIRE(floats_out != nullptr, "ppoaf_lstm2_workspace_floats: floats_out is NULL");
    const Lstm2Layout L = layout2_of(*d);
    floats_out[0] = L.total;
    floats_out[1] = L.size;
    return PPOAF_OK;
}

extern "C" int ppoaf_lstm2_forward(const ppoaf_lstm2_desc_t* d, const float* x, const float* h0, const float* c0,
                                   float* out, float* hn, float* cn, int32_t stash, ppoaf_stream_t stream) {
    if (int rc = check_lstm2_desc(d, stash != 0, "ppoaf_lstm2_forward")) return rc;
    PPOAF_REQUIRE(x && h0 && c0 && out, "ppoaf_lstm2_forward: x / h0 / c0 / out is NULL");
    Lstm2Args a = lstm2_args_of(d);
    a.x = x; a.h0 = h0; a.c0 = c0; a.out = out; a.hn = hn; a.cn = cn; a.stash = stash != 0;
    hipStream_t s = (hipStream_t)stream;
    return d->hidden == 32 ? launch_forward<32>(a, s) : d->hidden == 64 ? launch_forward<64>(a, s) : launch_forward<128>(a, s);
}

extern "C" int ppoaf_lstm2_backward(const ppoaf_lstm2_desc_t* d, const float* c0, const float* dout, ppoaf_stream_t stream) {
    if (int rc = check_lstm2_desc(d, true, "ppoaf_lstm2_backward")) return rc;
    PPOAF_REQUIRE(c0 && dout, "ppoaf_lstm2_backward: c0 / dout is NULL");
    Lstm2Args a = lstm2_args_of(d);
    a.c0 = c0; a.dout = dout;
    hipStream_t s = (hipStream_t)stream;
    return d->hidden == 32 ? launch_backward<32>(a, s) : d->hidden == 64 ? launch_backward<64>(a, s) : launch_backward<128>(a, s);
}

extern "C" int ppoaf_lstm2_wgrad(const ppoaf_lstm2_desc_t* d, const float* x, ppoaf_stream_t stream) {
    if (int rc = check_lstm2_desc(d, true, "ppoaf_lstm2_wgrad")) return rc;
    PPOAF_REQUIRE(x && d->grads, "ppoaf_lstm2_wgrad: x / grads is NULL");
    WJobs2 J{};
    const int nt = lstm2_wgrad_jobs(J, lstm2_args_of(d), d->hidden, x, d->grads);
    hipLaunchKernelGGL(lstm2_wgrad_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, J);
    return check_launch("ppoaf_lstm2_wgrad");
}
