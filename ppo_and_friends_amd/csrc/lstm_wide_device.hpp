// K18 for a 256-wide one-layer LSTM network: the forward and the backward (head, LayerNorm, BPTT) of one tile of 32 rows.
// The contract is lstm_rows_forward<H, false> / lstm_rows_backward<H> of lstm_device.hpp at H = 256 -- the same
// arguments (LstmArgs), the same bucket and workspace layout (layout_of), so the weight-gradient launch
// (lstm_wgrad_tile, generic in H) reads what these kernels stash.  The split is another one (see lstm_wide.hip):
//   * 32 rows per workgroup (two MFMA M tiles), 8 waves; wave w owns hidden units [32 w, 32 w + 32) of all four gates,
//     so a lane still holds i, f, g, o (forward) or dh, dc (backward) of the same (row, unit) pairs and the cell code
//     is lane-local; only the new h (forward) and the step's d gates (backward) cross waves, through LDS;
//   * W_hh (1 MiB) is streamed every step as WHOLE 128-byte lines and every fragment feeds both M tiles: the forward
//     asks for 8 rows x 128 bytes per instruction and turns the lines into fragment order in a wave-private LDS slot
//     (mfma_rows_x_lines' scheme); the backward needs B[k][unit] = W_hh[k][unit], whose 32 units of a wave ARE one
//     line of row k -- each lane takes two neighbouring units (8 bytes), which makes the wave's two N tiles the even
//     and the odd units: no reordering at all.
#pragma once
#include "lstm_device.hpp"

namespace ppoaf {

constexpr int kWH = 256;                  // the hidden width these bodies are written for
constexpr int kWRows = 32;                // rows per workgroup
constexpr int kWWaves = 8;
constexpr int kWThreads = 64 * kWWaves;
constexpr int kWHS = kWH + 4;             // LDS row stride of x, h and the head's first buffer
constexpr int kWGS = 4 * kWH + 4;         // LDS row stride of a step's d gates
// forward LDS, floats: x of one step | h, double-buffered | two line slots per wave (the head's buffers afterwards)
constexpr int kWFwdX = 0, kWFwdH = kWRows * kWHS, kWFwdSlots = kWFwdH + 2 * kWRows * kWHS;
constexpr int kWFwdLds = kWFwdSlots + kWWaves * 2 * kLineSlot;
static_assert(kWWaves * 2 * kLineSlot >= 2 * kWRows * kLFS, "the head's buffers reuse the line slots");
// backward LDS, floats: the d gates of one step (the head's buffers and d h_S before the first step)
constexpr int kWBwdLds = kWRows * kWGS;
static_assert(kWBwdLds >= 2 * kWRows * kLFS + kWRows * kWHS, "the head's buffers reuse the d gates' tile");

typedef unsigned ppoaf_u32x2 __attribute__((ext_vector_type(2)));

// One forward tile of W_hh -- 16 gate rows x 256 -- as 16 requests of 8 rows x 128 bytes: raw[2 q + h] = 16 bytes of row
// 8 h + lane / 8, line q, block lane % 8.  `off`: the lane's byte offset of (row 32 w + lane / 8, block lane % 8);
// `disp`: the tile's displacement (wave-uniform).
__device__ __forceinline__ void wide_request_tile(const __amdgpu_buffer_rsrc_t rs, const unsigned off, const int disp,
                                                  float4 (&raw)[16]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        raw[2 * q] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, disp + 128 * q, 0));
        raw[2 * q + 1] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, disp + 8 * kWH * 4 + 128 * q, 0));
    }
}

// z0 / z1 += A[rows 0..15 / 16..31, 256] . tile, the tile's lines going through the wave's two LDS slots into fragment
// order (three stages in flight: line q + 2 being written, line q + 1 read back, line q in the matrix pipe), and the
// tile at displacement `next` requested into `raw` line by line as the registers come free.  Four accumulators (row tile x even / odd chunk) keep the matrix pipe issuing back to back; the sums' order is fixed.
__device__ __forceinline__ void wide_rows_x_lines(const float* __restrict__ A, const int lane, float4 (&raw)[16],
                                                  float* __restrict__ scratch, f32x4& z0, f32x4& z1,
                                                  const __amdgpu_buffer_rsrc_t rs, const unsigned off, const int next) {
    constexpr int NL = 8;
    const float* ar0 = A + (lane & 15) * kWHS + 4 * (lane >> 4);
    const float* ar1 = ar0 + 16 * kWHS;
    float* wr = scratch + (lane >> 3) * kLineRow + 4 * (lane & 7);
    const float* rd = scratch + (lane & 15) * kLineRow + 4 * (lane >> 4);
    f32x4 p00 = z0, p10 = z1;
    f32x4 p01 = {0.f, 0.f, 0.f, 0.f}, p11 = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<float4*>(wr) = raw[0];
    *reinterpret_cast<float4*>(wr + 8 * kLineRow) = raw[1];
    *reinterpret_cast<float4*>(wr + kLineSlot) = raw[2];
    *reinterpret_cast<float4*>(wr + kLineSlot + 8 * kLineRow) = raw[3];
    __builtin_amdgcn_wave_barrier();                      // (LDS executes a wave's instructions in order)
    float4 f0 = *reinterpret_cast<const float4*>(rd);
    float4 f1 = *reinterpret_cast<const float4*>(rd + 16);
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int slot = (q & 1) * kLineSlot;
        // line q of this tile went to its slot two iterations ago: its registers take line q of the NEXT tile, a whole
        // tile's MFMAs ahead of its use
        raw[2 * q] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, next + 128 * q, 0));
        raw[2 * q + 1] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, next + 8 * kWH * 4 + 128 * q, 0));
        float4 g0 = f0, g1 = f1;
        if (q + 1 < NL) {
            g0 = *reinterpret_cast<const float4*>(rd + (kLineSlot - slot));
            g1 = *reinterpret_cast<const float4*>(rd + (kLineSlot - slot) + 16);
        }
        const float4 a00 = *reinterpret_cast<const float4*>(ar0 + 32 * q);
        const float4 a01 = *reinterpret_cast<const float4*>(ar0 + 32 * q + 16);
        const float4 a10 = *reinterpret_cast<const float4*>(ar1 + 32 * q);
        const float4 a11 = *reinterpret_cast<const float4*>(ar1 + 32 * q + 16);
        p00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a00.x, f0.x, p00, 0, 0, 0);
        p10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a10.x, f0.x, p10, 0, 0, 0);
        p01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a01.x, f1.x, p01, 0, 0, 0);
        p11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a11.x, f1.x, p11, 0, 0, 0);
        p00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a00.y, f0.y, p00, 0, 0, 0);
        p10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a10.y, f0.y, p10, 0, 0, 0);
        p01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a01.y, f1.y, p01, 0, 0, 0);
        p11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a11.y, f1.y, p11, 0, 0, 0);
        p00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a00.z, f0.z, p00, 0, 0, 0);
        p10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a10.z, f0.z, p10, 0, 0, 0);
        p01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a01.z, f1.z, p01, 0, 0, 0);
        p11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a11.z, f1.z, p11, 0, 0, 0);
        p00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a00.w, f0.w, p00, 0, 0, 0);
        p10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a10.w, f0.w, p10, 0, 0, 0);
        p01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a01.w, f1.w, p01, 0, 0, 0);
        p11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a11.w, f1.w, p11, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
        if (q + 2 < NL) {                                 // this line's slot is free: its fragments were read an iteration ago
            *reinterpret_cast<float4*>(wr + slot) = raw[2 * q + 4];
            *reinterpret_cast<float4*>(wr + slot + 8 * kLineRow) = raw[2 * q + 5];
        }
        f0 = g0; f1 = g1;
        __builtin_amdgcn_sched_barrier(0);                // (one line's reads in flight, not all eight: the registers are the budget)
    }
    z0 = p00 + p01;
    z1 = p10 + p11;
}

// Rows [32 g, 32 g + 32) of the network: S recurrent steps, LayerNorm, activation, feed-forward head; `lds`: kWFwdLds
// floats.  In tile i = 2 q + u (gate q, half u of the wave's units) lane column c is unit 32 w + 16 u + c.
// STEP = false (K18): the outputs go to a.out; nullptr is returned.  STEP = true (K21 at 256, lstm_wide_step.hip): the
// contract of lstm_rows_forward<H, true, XRows> -- one step (S is 1 whatever a.S says, so the time loop folds away), the
// input rows come through XRows, the last Linear's rows stay in LDS (the returned pointer, row stride kLFS, valid for
// every thread after the call) for the one-lane-per-row heads, the final (h, c) also go to a.hn_row / a.cn_row, a.hn /
// a.cn are written only when *a.commit says so, and nothing is stashed.  There a.hn / a.cn may be a.h0 / a.c0: a
// workgroup reads only its own 32 rows of them -- h into LDS, c into registers, both ahead of the first __syncthreads --
// and writes them after the cell.  Both forms add in one order (bias, the x . W_ih chunks, the eight lines with the
// even- and odd-chunk accumulators summed last), so a step's states are bitwise those of a one-step K18 call.
template <bool STEP, class XRows = LstmXDense>
__device__ __forceinline__ const float* lstm_wide_rows_forward(const LstmArgs& a, const int g_tile, float* __restrict__ lds,
                                                               const XRows xrows = XRows()) {
    constexpr int H = kWH, HS = kWHS, NT = kWThreads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, s4 = lane >> 4, c16 = lane & 15;
    const long r0 = (long)g_tile * kWRows;
    const long N = a.N;
    const int S = STEP ? 1 : a.S, I = a.I, Ip = (a.I + 15) & ~15;
    float* xs = lds + kWFwdX;
    float* hs = lds + kWFwdH;
    float* slots = lds + kWFwdSlots + w * 2 * kLineSlot;
    const float* Wih = a.P + a.L.w_ih;
    const __amdgpu_buffer_rsrc_t rs = frag_rsrc(a.P + a.L.w_hh);
    const unsigned off = (unsigned)(((32 * w + (lane >> 3)) * H + 4 * (lane & 7)) * 4);
    auto disp_of = [](int i) { return (((i >> 1) * H + 16 * (i & 1)) * H) * 4; };

    float bias[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int col = (i >> 1) * H + 32 * w + 16 * (i & 1) + c16;
        bias[i] = a.P[a.L.b_ih + col] + a.P[a.L.b_hh + col];
    }
    auto load_x = [&](int t) {
        for (int e = tid; e < kWRows * Ip; e += NT) {
            const int r = e / Ip, k = e - r * Ip;
            const long n = r0 + r;
            xs[r * HS + k] = (n < N && k < I) ? xrows.load(a, n, S, t, I, k) : 0.f;
        }
    };
    float4 raw[16];
    constexpr int kHLoads = kWRows * H / NT;              // h values a thread stages
    [[maybe_unused]] float hv[STEP ? kHLoads : 1];
    if constexpr (STEP) {
        // one step: no step before hides the first tile's latency, so the tile is asked for ahead of the h / c / x loads,
        // and a thread's h loads are all issued before the first is stored (one round trip under the tile's, not 16)
        wide_request_tile(rs, off, disp_of(0), raw);
        __builtin_amdgcn_sched_barrier(0);                // (the scheduler would sink the request behind the staging)
#pragma unroll
        for (int q = 0; q < kHLoads; ++q) {
            const int e = tid + q * NT, r = e / H, k = e - r * H;
            const long n = r0 + r;
            hv[q] = n < N ? a.h0[n * H + k] : 0.f;
        }
    } else {
        for (int e = tid; e < kWRows * H; e += NT) {
            const int r = e / H, k = e - r * H;
            const long n = r0 + r;
            hs[r * HS + k] = n < N ? a.h0[n * H + k] : 0.f;
        }
    }
    float cr[2][2][4];                                    // c of (half u, row tile m, row 4 s4 + g)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long n = r0 + 16 * m + 4 * s4 + g;
                cr[u][m][g] = n < N ? a.c0[n * H + 32 * w + 16 * u + c16] : 0.f;
            }
    if constexpr (STEP) {
#pragma unroll
        for (int q = 0; q < kHLoads; ++q) {
            const int e = tid + q * NT, r = e / H;
            hs[r * HS + (e - r * H)] = hv[q];
        }
    }
    load_x(0);
    if constexpr (!STEP)
        wide_request_tile(rs, off, disp_of(0), raw);      // (the weights do not change: the first tile of a step is asked
    __syncthreads();                                      //  for during the last tile of the step before, across the barriers)

    for (int t = 0; t < S; ++t) {
        const float* hb = hs + (t & 1) * kWRows * HS;
        f32x4 z[8][2];
        // input projection: x_t . W_ih^T on top of the biases (fragment loads: a row of W_ih is I floats, no line grid)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x4 acc0 = {bias[i], bias[i], bias[i], bias[i]};
            f32x4 acc1 = acc0;
            const float* wrow = Wih + (unsigned)(((i >> 1) * H + 32 * w + 16 * (i & 1) + c16) * I);   // (< 2^18: one register)
#pragma unroll 1
            for (int c = 0; c < Ip / 16; ++c) {
                const int k0 = 16 * c + 4 * s4;
                const float4 x0 = *reinterpret_cast<const float4*>(xs + c16 * HS + k0);
                const float4 x1 = *reinterpret_cast<const float4*>(xs + (16 + c16) * HS + k0);
                const float b0 = k0 < I ? wrow[k0] : 0.f, b1 = k0 + 1 < I ? wrow[k0 + 1] : 0.f;
                const float b2 = k0 + 2 < I ? wrow[k0 + 2] : 0.f, b3 = k0 + 3 < I ? wrow[k0 + 3] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, b0, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, b1, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, b1, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, b2, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, b2, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, b3, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, b3, acc1, 0, 0, 0);
            }
            z[i][0] = acc0;
            z[i][1] = acc1;
        }
        __syncthreads();                                  // every wave has read x_t: the buffer takes x_{t+1}
        if (t + 1 < S) load_x(t + 1);
        // recurrent part: the eight tiles of the wave, tile i + 1 requested during the MFMAs of tile i
#pragma unroll
        for (int i = 0; i < 8; ++i)
            wide_rows_x_lines(hb, lane, raw, slots, z[i][0], z[i][1], rs, off, disp_of((i + 1) & 7));
        float* hnext = hs + ((t + 1) & 1) * kWRows * HS;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int rr = 16 * m + 4 * s4 + g, j = 32 * w + 16 * u + c16;
                    const long n = r0 + rr;
                    const float ig = sigm(z[u][m][g]), fg = sigm(z[2 + u][m][g]);
                    const float gg = tanhf(z[4 + u][m][g]), og = sigm(z[6 + u][m][g]);
                    const float c = fg * cr[u][m][g] + ig * gg;
                    const float h = og * tanhf(c);
                    cr[u][m][g] = c;
                    hnext[rr * HS + j] = h;
                    if (!STEP && a.stash && n < N) {
                        float* gp = a.ws + a.L.gates + (n * S + t) * 4 * H + j;
                        gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
                        a.ws[a.L.cst + (n * S + t) * H + j] = c;
                        a.ws[a.L.hst + (n * S + t) * H + j] = h;
                    }
                }
        __syncthreads();
    }
    const float* hfin = hs + (S & 1) * kWRows * HS;
    bool keep = true;
    if constexpr (STEP) keep = a.commit == nullptr || *a.commit != 0;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rr = 16 * m + 4 * s4 + g, j = 32 * w + 16 * u + c16;
                const long n = r0 + rr;
                if (n < N) {
                    if (a.hn && keep) a.hn[n * H + j] = hfin[rr * HS + j];
                    if (a.cn && keep) a.cn[n * H + j] = cr[u][m][g];
                    if constexpr (STEP) {
                        if (a.hn_row) a.hn_row[n * H + j] = hfin[rr * HS + j];
                        if (a.cn_row) a.cn_row[n * H + j] = cr[u][m][g];
                    }
                }
            }

    // ---- head: LayerNorm(256) -> activation -> Linear layers (x's buffer and the line slots are free now)
    float* A0 = xs;
    float* A1 = lds + kWFwdSlots;
    float* A2 = A1 + kWRows * kLFS;
    for (int r = w; r < kWRows; r += kWWaves) {
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
            if (!STEP && a.stash && n < N) a.ws[a.L.acts[0] + n * H + k] = y2;
        }
        if (!STEP && a.stash && n < N && lane == 0) { a.ws[a.L.stats + 2 * n] = mean; a.ws[a.L.stats + 2 * n + 1] = rstd; }
    }
    __syncthreads();
    // first Linear (256 -> F, never the last: depth >= 1) on the matrix pipe: wave w forms output columns [16 w, 16 w + 16)
    // of both row tiles from one set of fragments
    if (16 * w < a.F) {
        float4 fr[16];
        load_fwd_frags<16>(a.P + a.L.fw[0], 16 * w, lane, fr);
        const int mcol = 16 * w + c16;
        const float b = a.P[a.L.fb[0] + mcol];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f32x4 acc = mfma_rows_x_frags<16>(A0 + 16 * m * HS, HS, lane, fr, b);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rr = 16 * m + 4 * s4 + g;
                const long n = r0 + rr;
                const float sv = act_fwd(acc[g], a.act);
                A1[rr * kLFS + mcol] = sv;
                if (!STEP && a.stash && n < N) a.ws[a.L.acts[1] + n * a.F + mcol] = sv;
            }
        }
    }
    __syncthreads();
    const float* in = A1;
    for (int l = 1; l <= a.D; ++l) {
        const bool last = l == a.D;
        const int M = last ? a.O : a.F, K = a.F;
        float* ob = (l & 1) ? A2 : A1;
        const float* W = a.P + a.L.fw[l];
        const float* b = a.P + a.L.fb[l];
        for (int e = tid; e < kWRows * M; e += NT) {
            const int r = e / M, m = e - r * M;
            const long n = r0 + r;
            const float* ir = in + r * kLFS;
            const float* wr = W + (long)m * K;
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += ir[k] * wr[k];
            s += b[m];
            if (last) {
                if constexpr (STEP) ob[r * kLFS + m] = s;
                else if (n < N) a.out[n * M + m] = s;
            } else {
                s = act_fwd(s, a.act);
                ob[r * kLFS + m] = s;
                if (!STEP && a.stash && n < N) a.ws[a.L.acts[l + 1] + n * M + m] = s;
            }
        }
        __syncthreads();
        in = ob;
    }
    return STEP ? in : nullptr;
}

// One group of the backward stream: chunks [8 grp, 8 grp + 8) of the 64 chunks of 16 gate rows.  fr[4 c + j] = the two units
// (32 w + 2 (lane & 15), + 1) of row 16 (8 grp + c) + 4 (lane >> 4) + j: an instruction reads 4 rows x 128 bytes.
__device__ __forceinline__ void wide_request_dgrad(const __amdgpu_buffer_rsrc_t rs, const unsigned off, const int grp,
                                                   float2 (&fr)[32]) {
    const int base = grp * 8 * 16 * kWH * 4;
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const ppoaf_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, base + (16 * c + j) * kWH * 4, 0);
            fr[4 * c + j] = make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
        }
}

// acc[m][u] += G[rows of tile m, the group's 128 gate columns] . the group's fragments (u: even / odd units of the wave)
__device__ __forceinline__ void wide_dgates_x_frags(const float* __restrict__ G, const int lane, const int grp,
                                                    const float2 (&fr)[32], f32x4 (&acc)[2][2]) {
    const float* g0 = G + (lane & 15) * kWGS + 128 * grp + 4 * (lane >> 4);
    const float* g1 = g0 + 16 * kWGS;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 a0 = *reinterpret_cast<const float4*>(g0 + 16 * c);
        const float4 a1 = *reinterpret_cast<const float4*>(g1 + 16 * c);
        const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[j], fr[4 * c + j].x, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[j], fr[4 * c + j].x, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[j], fr[4 * c + j].y, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[j], fr[4 * c + j].y, acc[1][1], 0, 0, 0);
        }
    }
}

// The backward of rows [32 g, 32 g + 32) through the head, LayerNorm and time: d out -> the pre-activation gradients of
// every Linear, of the LayerNorm output and of every (row, step)'s gates, into the workspace the forward stashed into
// (a.ws: 8-byte aligned, checked by the launcher).  `lds`: kWBwdLds floats.  Lane column c of N tile u is unit
// 32 w + 2 c + u.
__device__ __forceinline__ void lstm_wide_rows_backward(const LstmArgs& a, const int g_tile, float* __restrict__ lds) {
    constexpr int H = kWH, HS = kWHS, GS = kWGS, NT = kWThreads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, s4 = lane >> 4, c16 = lane & 15;
    const long r0 = (long)g_tile * kWRows;
    const long N = a.N;
    const int S = a.S, F = a.F, D = a.D, O = a.O;
    const int j2 = 32 * w + 2 * c16;                       // the lane's unit pair (j2, j2 + 1)
    float* ws = a.ws;

    // ---- head: d logits -> d pre-activation of every Linear -> d LayerNorm output -> d h_S.  Scalar sums: at most
    // 32 x 256 outputs of F <= 128 terms over 512 threads, once per window, against S steps of 1024 MFMAs per wave.
    float* Bc = lds;
    float* Bn = lds + kWRows * kLFS;
    float* DH = lds + 2 * kWRows * kLFS;
    for (int e = tid; e < kWRows * O; e += NT) {
        const int r = e / O, o = e - r * O;
        const long n = r0 + r;
        const float v = n < N ? a.dout[n * O + o] : 0.f;
        Bc[r * kLFS + o] = v;
        if (n < N) ws[a.L.dz[D] + n * O + o] = v;
    }
    __syncthreads();
    for (int l = D; l >= 0; --l) {
        const int M = l == D ? O : F, K = l == 0 ? H : F;
        const float* W = a.P + a.L.fw[l];
        for (int e = tid; e < kWRows * K; e += NT) {
            const int r = e / K, k = e - r * K;
            const long n = r0 + r;
            float s = 0.f;
            for (int m = 0; m < M; ++m) s += Bc[r * kLFS + m] * W[(long)m * K + k];
            const float av = n < N ? ws[a.L.acts[l] + n * K + k] : 0.f;
            const float g = n < N ? s * act_bwd(av, a.act) : 0.f;
            if (l > 0) {
                Bn[r * kLFS + k] = g;
                if (n < N) ws[a.L.dz[l - 1] + n * F + k] = g;
            } else {
                DH[r * HS + k] = g;
                if (n < N) ws[a.L.dy + n * H + k] = g;
            }
        }
        __syncthreads();
        float* t = Bc; Bc = Bn; Bn = t;
    }
    for (int r = w; r < kWRows; r += kWWaves) {
        const long n = r0 + r;
        if (n >= N) {
            for (int k = lane; k < H; k += 64) DH[r * HS + k] = 0.f;
            continue;
        }
        const float mean = ws[a.L.stats + 2 * n], rstd = ws[a.L.stats + 2 * n + 1];
        const float* hS = ws + a.L.hst + (n * S + S - 1) * H;
        float xh[4], gy[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = lane + 64 * u;
            xh[u] = (hS[k] - mean) * rstd;
            gy[u] = DH[r * HS + k] * a.P[a.L.ln_w + k];
            s1 += gy[u];
            s2 += gy[u] * xh[u];
            ws[a.L.xhat + n * H + k] = xh[u];
        }
        s1 = wave_sum(s1) / (float)H;
        s2 = wave_sum(s2) / (float)H;
#pragma unroll
        for (int u = 0; u < 4; ++u) DH[r * HS + lane + 64 * u] = rstd * (gy[u] - s1 - xh[u] * s2);
    }
    __syncthreads();
    f32x4 dh[2][2];                                        // (row tile m, unit j2 + u), rows 4 s4 + g
    float dc[2][2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float2 v = *reinterpret_cast<const float2*>(DH + (16 * m + 4 * s4 + g) * HS + j2);
            dh[m][0][g] = v.x; dh[m][1][g] = v.y;
            dc[m][0][g] = dc[m][1][g] = 0.f;
        }
    const __amdgpu_buffer_rsrc_t rs = frag_rsrc(a.P + a.L.w_hh);
    const unsigned off = (unsigned)((4 * s4 * H + j2) * 4);
    float2 frA[32], frB[32];
    __syncthreads();                                       // d h_S shares the LDS with the d gates

    for (int t = S - 1; t >= 0; --t) {
        if (t > 0) wide_request_dgrad(rs, off, 0, frA);    // ahead of the cell code and the barrier
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rr = 16 * m + 4 * s4 + g;
                const long n = r0 + rr;
                float2 da[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) da[q] = make_float2(0.f, 0.f);
                if (n < N) {
                    const float* gp = ws + a.L.gates + (n * S + t) * 4 * H + j2;
                    float2 gate[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) gate[q] = *reinterpret_cast<const float2*>(gp + q * H);
                    const float2 ct = *reinterpret_cast<const float2*>(ws + a.L.cst + (n * S + t) * H + j2);
                    float2 cp;
                    if (t > 0) cp = *reinterpret_cast<const float2*>(ws + a.L.cst + (n * S + t - 1) * H + j2);
                    else cp = make_float2(a.c0[n * H + j2], a.c0[n * H + j2 + 1]);
                    const float ctv[2] = {ct.x, ct.y}, cpv[2] = {cp.x, cp.y};
                    float o4[4][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const float ig = u ? gate[0].y : gate[0].x, fg = u ? gate[1].y : gate[1].x;
                        const float gg = u ? gate[2].y : gate[2].x, og = u ? gate[3].y : gate[3].x;
                        const float tc = tanhf(ctv[u]);
                        const float dhv = dh[m][u][g];
                        const float dcv = dc[m][u][g] + dhv * og * (1.f - tc * tc);
                        o4[0][u] = dcv * gg * (ig * (1.f - ig));
                        o4[1][u] = dcv * cpv[u] * (fg * (1.f - fg));
                        o4[2][u] = dcv * ig * (1.f - gg * gg);
                        o4[3][u] = dhv * tc * (og * (1.f - og));
                        dc[m][u][g] = dcv * fg;
                    }
                    float* dp = ws + a.L.dG + (n * S + t) * 4 * H + j2;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        da[q] = make_float2(o4[q][0], o4[q][1]);
                        *reinterpret_cast<float2*>(dp + q * H) = da[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<float2*>(lds + rr * GS + q * H + j2) = da[q];
            }
        __syncthreads();
        if (t > 0) {
            // d h_{t-1} = d gates . W_hh: 8 groups of 8 chunks, group i + 1 requested ahead of the MFMAs of group i
            f32x4 acc[2][2];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[m][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int p = 0; p < 4; ++p) {
                wide_request_dgrad(rs, off, 2 * p + 1, frB);
                wide_dgates_x_frags(lds, lane, 2 * p, frA, acc);
                if (p < 3) wide_request_dgrad(rs, off, 2 * p + 2, frA);
                wide_dgates_x_frags(lds, lane, 2 * p + 1, frB, acc);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int u = 0; u < 2; ++u) dh[m][u] = acc[m][u];
            __syncthreads();                               // the tile takes the next step's d gates
        }
    }
}

// host: the launchers of lstm_wide.hip, called by the K18 entry points of lstm.hip at hidden == 256
int lstm_wide_forward(const LstmArgs& a, hipStream_t stream);
int lstm_wide_backward(const LstmArgs& a, hipStream_t stream);

}  // namespace ppoaf
