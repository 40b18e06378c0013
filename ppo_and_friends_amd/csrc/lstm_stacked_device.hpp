// What the two-layer LSTM kernels share: K18 for two stacked layers (lstm_stacked.hip) and the one-launch rollout /
// evaluation step of such a pair (lstm_stacked_step.hip).  Descriptor check, bucket and workspace layout, kernel
// arguments, the streamed fragment loaders and the cell update -- one copy of each, so a step of the one-launch kernel
// and a one-step call of ppoaf_lstm2_forward run the same cell code on the same sums.
#pragma once
#include "lstm_device.hpp"

namespace ppoaf {
namespace {

#define PPOAF_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

constexpr int kL2MaxJobs = 16;                   // weight-gradient jobs of one two-layer network (14) and a log_std job

// Streamed weight fragments through ONE buffer resource per matrix: every load of the kernel shares one per-lane byte
// offset and the block's displacement rides in the scalar / immediate offset, so no 64-bit address pair per load is kept
// across the steps (as global loads the loop-invariant addresses of a step's loads -- 64 forward, 128 dgrad -- took more
// registers than the kernel has and went to the private segment).  The fragments are load_fwd_frags_ld's / load_dgrad_frags_ld's.
template <int KC>
__device__ __forceinline__ void load_fwd_frags_rs(const __amdgpu_buffer_rsrc_t rs, const unsigned off, const int disp, float4 (&fr)[KC]) {
#pragma unroll
    for (int c = 0; c < KC; c += 2) fr[c] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, disp + 64 * c, 0));
    __builtin_amdgcn_sched_barrier(0);                    // (even chunks first: see load_fwd_frags)
#pragma unroll
    for (int c = 1; c < KC; c += 2) fr[c] = frag_u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, disp + 64 * c, 0));
}
template <int KC>
__device__ __forceinline__ void load_dgrad_frags_rs(const __amdgpu_buffer_rsrc_t rs, const unsigned off, const int k0, const int row, float4 (&fr)[KC]) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const int d = (k0 + 16 * c) * row;
        fr[c] = make_float4(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, d, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, d + row, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, d + 2 * row, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, d + 3 * row, 0)));
    }
}

struct Lstm2Layout {
    // parameters, float offsets into the network's bucket (module order, each tensor padded to 4 floats)
    long w_ih[2], w_hh[2], b_ih[2], b_hh[2], ln_w, ln_b, fw[3], fb[3], size;
    // workspace, float offsets
    long gates[2], cst[2], hst[2], hinit[2], stats, acts[3], dG[2], dh0, dy, xhat, dz[3], total;
};

Lstm2Layout layout2_of(const ppoaf_lstm2_desc_t& d) {
    Lstm2Layout L{};
    const long I = d.in_dim, H = d.hidden, F = d.ff_hidden, O = d.out_dim, D = d.ff_depth;
    long o = 0;
    for (int l = 0; l < 2; ++l) {
        L.w_ih[l] = o; o += pad4(4 * H * (l == 0 ? I : H));
        L.w_hh[l] = o; o += pad4(4 * H * H);
        L.b_ih[l] = o; o += pad4(4 * H);
        L.b_hh[l] = o; o += pad4(4 * H);
    }
    L.ln_w = o; o += pad4(H);
    L.ln_b = o; o += pad4(H);
    for (long l = 0; l <= D; ++l) {
        const long in = l == 0 ? H : F, out = l == D ? O : F;
        L.fw[l] = o; o += pad4(out * in);
        L.fb[l] = o; o += pad4(out);
    }
    L.size = o;
    const long R = d.rows, S = d.steps;
    long w = 0;
    for (int l = 0; l < 2; ++l) {
        L.gates[l] = w; w += R * S * 4 * H;   // activated i, f, g, o per (row, step)
        L.cst[l] = w; w += R * S * H;         // c_t
        L.hst[l] = w; w += R * S * H;         // h_t
        L.hinit[l] = w; w += R * H;           // the initial h, dense (what the weight gradients read at t = 0)
    }
    L.stats = w; w += R * 2;                  // LayerNorm mean, 1 / std
    L.acts[0] = w; w += R * H;                // activation(LayerNorm(h1_S))
    for (long l = 1; l <= D; ++l) { L.acts[l] = w; w += R * F; }
    for (int l = 0; l < 2; ++l) { L.dG[l] = w; w += R * S * 4 * H; }    // d pre-activation gates
    L.dh0 = w; w += R * S * H;                // d h0_t through W_ih_l1
    L.dy = w; w += R * H;                     // d LayerNorm output
    L.xhat = w; w += R * H;                   // normalised h1_S
    for (long l = 0; l <= D; ++l) { L.dz[l] = w; w += R * (l == D ? O : F); }
    L.total = w;
    return L;
}

struct Lstm2Args {
    const float* P;
    float* ws;
    const float* x;
    const float* h0;
    const float* c0;
    float* out;
    float* hn;
    float* cn;
    const float* dout;
    long N, rs, ls;               // rows; row and layer stride of the states
    int S, I, F, D, O, act, stash;
    Lstm2Layout L;
};

int check_lstm2_desc(const ppoaf_lstm2_desc_t* d, bool need_ws, const char* what) {
    PPOAF_REQUIRE(d != nullptr, "%s: desc / params is NULL", what);
    ppoaf_lstm_desc_t one{};
    one.in_dim = d->in_dim; one.hidden = d->hidden; one.ff_hidden = d->ff_hidden; one.ff_depth = d->ff_depth;
    one.out_dim = d->out_dim; one.activation = d->activation; one.rows = d->rows; one.steps = d->steps;
    one.params = d->params;
    if (int rc = check_lstm_desc(&one, false, what)) return rc;         // the one-layer limits and their words
    const long H = d->hidden, rs = d->state_row_stride, ls = d->state_layer_stride;
    PPOAF_REQUIRE((rs == H && ls == d->rows * H) || (rs == 2 * H && ls == H),
                  "%s: state strides (row %ld, layer %ld) describe neither [2, rows, %ld] nor [rows, 2, %ld]", what, rs, ls, H, H);
    if (need_ws) {
        const Lstm2Layout L = layout2_of(*d);
        PPOAF_REQUIRE(d->workspace != nullptr && d->workspace_floats >= L.total,
                      "%s: workspace holds %lld floats, %ld needed", what, (long long)d->workspace_floats, L.total);
    }
    return PPOAF_OK;
}

Lstm2Args lstm2_args_of(const ppoaf_lstm2_desc_t* d) {
    Lstm2Args a{};
    a.P = d->params;
    a.ws = d->workspace;
    a.N = d->rows;
    a.rs = d->state_row_stride;
    a.ls = d->state_layer_stride;
    a.S = (int)d->steps;
    a.I = d->in_dim;
    a.F = d->ff_hidden;
    a.D = d->ff_depth;
    a.O = d->out_dim;
    a.act = d->activation;
    a.L = layout2_of(*d);
    return a;
}

// i, f, g, o pre-activations of this lane's four (row, unit) pairs -> the cell update; the new h goes to `hnext` (LDS)
// and, with stash, the activated gates, c and h to the workspace planes of the layer.
template <int H>
__device__ __forceinline__ void lstm2_cell(const Lstm2Args& a, const f32x4 (&z)[4], float (&cr)[4], float (&hr)[4], float* hnext,
                                           const long gates, const long cst, const long hst, const long r0, const int t,
                                           const int j, const int lane) {
    constexpr int HS = H + 4;
    // wave-uniform bases of the tile's step-t planes, 32-bit lane offsets: no address pair per store kept across the steps
    float* gbase = a.ws + gates + (r0 * a.S + t) * 4 * H;
    float* cbase = a.ws + cst + (r0 * a.S + t) * H;
    float* hbase = a.ws + hst + (r0 * a.S + t) * H;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int rr = 4 * (lane >> 4) + g;
        const long n = r0 + rr;
        const float ig = sigm(z[0][g]), fg = sigm(z[1][g]), gg = tanhf(z[2][g]), og = sigm(z[3][g]);
        const float c = fg * cr[g] + ig * gg;
        const float h = og * tanhf(c);
        cr[g] = c;
        hr[g] = h;
        hnext[rr * HS + j] = h;
        if (a.stash && n < a.N) {
            float* gp = gbase + (unsigned)(rr * a.S * 4 * H + j);
            gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
            cbase[(unsigned)(rr * a.S * H + j)] = c;
            hbase[(unsigned)(rr * a.S * H + j)] = h;
        }
    }
}

// Rows [16 g, 16 g + 16) of the two-layer network by a workgroup of 2 H / 16 waves: the wavefront of lstm_stacked.hip's
// header comment, LayerNorm, activation, feed-forward head.  ppoaf_lstm2_forward's kernel and the forward launch of the
// stacked update epoch (lstm_stacked_update.hip) both instantiate it, so both form the same sums in the same order.
// STEP = false: the outputs go to a.out.  STEP = true: they stay in LDS -- the returned pointer, row stride kLFS, valid
// after the call for every thread.  The body carries the calling kernels' PPOAF_NO_PK_F32, so it is compiled as it was
// inside ppoaf_lstm2_forward's kernel.
template <int H, bool STEP>
__device__ __forceinline__ PPOAF_NO_PK_F32 const float* lstm2_rows_forward(const Lstm2Args a, const unsigned g_tile) {
    constexpr int HT = H / 16, NW = 2 * HT, NT = NW * 64, HS = H + 4, XS = kLMaxIn + 4;
    static_assert(2 * kLRows * XS >= kLRows * HS + 2 * kLRows * kLFS, "head buffers reuse the x buffers");
    __shared__ float xs[2 * kLRows * XS];
    __shared__ float h0s[2][kLRows * HS];
    __shared__ float h1s[2][kLRows * HS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the layer branches below are whole-wave branches
    const bool upper = w >= HT;                               // wave-uniform: this wave works on layer 1
    const int wl = upper ? w - HT : w;
    const long r0 = (long)g_tile * kLRows;
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
                if constexpr (STEP) ob[r * kLFS + m] = s;
                else if (n < N) a.out[n * M + m] = s;
            } else {
                s = act_fwd(s, a.act);
                ob[r * kLFS + m] = s;
                if (a.stash && n < N) a.ws[acts + n * M + m] = s;
            }
        }
        __syncthreads();
        in = ob; IS = kLFS; K = M;
    }
    return in;
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

// The backward of rows [16 g, 16 g + 16) by a workgroup of H / 16 waves, the layers in turn (lstm_stacked.hip's header
// comment): a.dout -> the pre-activation gradients of the head, LayerNorm and both layers' gates, into the workspace the
// forward stashed into.  ppoaf_lstm2_backward's kernel and the backward launch of the stacked update epoch instantiate it.
template <int H>
__device__ __forceinline__ PPOAF_NO_PK_F32 void lstm2_rows_backward(const Lstm2Args a, const unsigned g_tile) {
    constexpr int HT = H / 16, NT = HT * 64, HS = H + 4, GS = 4 * H + 4;
    constexpr int kLds = 2 * kLRows * GS > 2 * kLRows * kLFS + kLRows * HS ? 2 * kLRows * GS : 2 * kLRows * kLFS + kLRows * HS;
    __shared__ float lds[kLds];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = (long)g_tile * kLRows;
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

// host: every weight-gradient job of the two-layer network (x [N, S, I]: what its forward read, G its gradient bucket)
// appended to jobs[n..]; tiles are numbered from tile_begin.  Returns the tile count after them.
int lstm2_wgrad_add_jobs(WJob* jobs, int& n, const int tile_begin, const Lstm2Args& a, const int H, const float* x, float* G) {
    const Lstm2Layout& L = a.L;
    const long N = a.N, S = a.S, NS = N * S;
    const int I = a.I, F = a.F, D = a.D, O = a.O;
    const float* ws = a.ws;
    int nt = tile_begin;
    auto add = [&](const float* A, int lda, const float* B, int ldb, const float* B0, int M, int Nc, int mode,
                   long K, float* out, float* out2, int ldo) {
        WJob& jb = jobs[n++];
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

}  // namespace
}  // namespace ppoaf
