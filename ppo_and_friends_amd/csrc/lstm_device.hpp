// The forward of the one-layer LSTM network (LSTMNetwork.forward_logits, networks/ppo_networks/lstm.py:103-127) for one
// tile of 16 rows, shared by K18 (lstm.hip: rollout step and training window) and K21 (lstm_policy_step.hip: the fused
// rollout / evaluation step, always S = 1): descriptor checks, bucket and workspace layout, kernel arguments and the
// workgroup body.  Both kernels instantiate lstm_rows_forward, so a step of K21 and a one-step call of K18 form the
// same sums in the same order.
// K22 (lstm_update.hip: the fused update mini-batch) instantiates the forward body too, and with it the backward body
// (lstm_rows_backward) and the weight-gradient tile body and job list (lstm_wgrad_tile, lstm_wgrad_add_jobs) that K18's
// own kernels run: one copy of each, so K18 and K22 form the same sums in the same order.
#pragma once
#include "common.hpp"
#include "mlp_device.hpp"

namespace ppoaf {

constexpr int kLRows = 16;                // rows per workgroup
constexpr int kLMaxIn = 256;
constexpr int kLMaxF = 128;
constexpr int kLFS = kLMaxF + 4;          // LDS row stride of the head's buffers
constexpr int kLMaxJobs = 12;

inline long pad4(long n) { return (n + 3) / 4 * 4; }

struct LstmLayout {
    // parameters, float offsets into the network's bucket (module order, each tensor padded to 4 floats)
    long w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, fw[3], fb[3], size;
    // workspace, float offsets
    long gates, cst, hst, stats, acts[3], dG, dy, xhat, dz[3], total;
};

inline LstmLayout layout_of(const ppoaf_lstm_desc_t& d) {
    LstmLayout L{};
    const long I = d.in_dim, H = d.hidden, F = d.ff_hidden, O = d.out_dim, D = d.ff_depth;
    long o = 0;
    L.w_ih = o; o += pad4(4 * H * I);
    L.w_hh = o; o += pad4(4 * H * H);
    L.b_ih = o; o += pad4(4 * H);
    L.b_hh = o; o += pad4(4 * H);
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
    L.gates = w; w += R * S * 4 * H;      // activated i, f, g, o per (row, step)
    L.cst = w; w += R * S * H;            // c_t
    L.hst = w; w += R * S * H;            // h_t
    L.stats = w; w += R * 2;              // LayerNorm mean, 1 / std
    L.acts[0] = w; w += R * H;            // activation(LayerNorm(h_S))
    for (long l = 1; l <= D; ++l) { L.acts[l] = w; w += R * F; }    // hidden layer outputs (post-activation)
    L.dG = w; w += R * S * 4 * H;         // d pre-activation gates
    L.dy = w; w += R * H;                 // d LayerNorm output
    L.xhat = w; w += R * H;               // normalised h_S
    for (long l = 0; l <= D; ++l) { L.dz[l] = w; w += R * (l == D ? O : F); }   // d pre-activation output of layer l
    L.total = w;
    return L;
}

struct LstmArgs {
    const float* P;
    float* ws;
    const float* x;
    const float* h0;
    const float* c0;
    float* out;
    float* hn;
    float* cn;
    const float* dout;
    long N;
    int S, I, F, D, O, act, stash;
    LstmLayout L;
    // K21 only (lstm_rows_forward<H, true>): second copies of the final (h, c) -- the step's rows of the rollout buffer --
    // and the device byte that decides whether hn / cn are written at all (NULL: they are)
    float* hn_row;
    float* cn_row;
    const unsigned char* commit;
};

inline int check_lstm_desc(const ppoaf_lstm_desc_t* d, bool need_ws, const char* what) {
    PPOAF_REQUIRE(d != nullptr && d->params != nullptr, "%s: desc / params is NULL", what);
    PPOAF_REQUIRE(d->hidden == 32 || d->hidden == 64 || d->hidden == 128, "%s: hidden %d not in {32, 64, 128}", what, d->hidden);
    PPOAF_REQUIRE(d->ff_hidden == 16 || d->ff_hidden == 32 || d->ff_hidden == 64 || d->ff_hidden == 128,
                  "%s: ff_hidden %d not in {16, 32, 64, 128}", what, d->ff_hidden);
    PPOAF_REQUIRE(d->ff_depth == 1 || d->ff_depth == 2, "%s: ff_depth %d not in {1, 2}", what, d->ff_depth);
    PPOAF_REQUIRE(d->in_dim >= 1 && d->in_dim <= kLMaxIn, "%s: in_dim %d not in [1, %d]", what, d->in_dim, kLMaxIn);
    PPOAF_REQUIRE(d->out_dim >= 1 && d->out_dim <= 8, "%s: out_dim %d not in [1, 8]", what, d->out_dim);
    PPOAF_REQUIRE(d->steps >= 1 && d->steps <= 16, "%s: steps %lld not in [1, 16]", what, (long long)d->steps);
    PPOAF_REQUIRE(d->rows >= 1, "%s: rows must be >= 1", what);
    PPOAF_REQUIRE(d->activation == PPOAF_ACT_RELU || d->activation == PPOAF_ACT_LEAKY_RELU || d->activation == PPOAF_ACT_TANH,
                  "%s: unknown activation %d", what, d->activation);
    if (need_ws) {
        const LstmLayout L = layout_of(*d);
        PPOAF_REQUIRE(d->workspace != nullptr && d->workspace_floats >= L.total,
                      "%s: workspace holds %lld floats, %ld needed", what, (long long)d->workspace_floats, L.total);
    }
    return PPOAF_OK;
}

inline LstmArgs lstm_args_of(const ppoaf_lstm_desc_t* d) {
    LstmArgs a{};
    a.P = d->params;
    a.ws = d->workspace;
    a.N = d->rows;
    a.S = (int)d->steps;
    a.I = d->in_dim;
    a.F = d->ff_hidden;
    a.D = d->ff_depth;
    a.O = d->out_dim;
    a.act = d->activation;
    a.L = layout_of(*d);
    return a;
}

__device__ __forceinline__ float sigm(float z) { return 1.f / (1.f + expf(-z)); }

// Where lstm_rows_forward finds element k of step t of row n of its input.  LstmXDense: a.x [N, S, I], the form K18, K22
// and the tensor form of K21 instantiate -- an empty object whose load() is the expression the staging loop has always
// held, so those instantiations keep their code.  LstmXBlocks (the block form of K21, always S = 1): the rows lie in a
// table of up to PPOAF_ROW_BLOCKS_MAX row blocks of `rows_per_block` rows each, row n being row n % rows_per_block of
// block n / rows_per_block; a 16-row tile may straddle blocks, so the address is formed per row.  N <= 2^27 (checked by
// the entry point), so the division is a 32-bit one.
struct LstmXDense {
    __device__ __forceinline__ float load(const LstmArgs& a, long n, int S, int t, int I, int k) const {
        return a.x[(n * S + t) * I + k];
    }
};
struct LstmXBlocks {
    const float* const* blocks;      // (points into the kernel arguments)
    unsigned rows_per_block;
    __device__ __forceinline__ const float* row(const long n, const int I) const {
        const unsigned b = (unsigned)n / rows_per_block;
        return blocks[b] + (long)((unsigned)n - b * rows_per_block) * I;
    }
    __device__ __forceinline__ float load(const LstmArgs&, long n, int, int, int I, int k) const { return row(n, I)[k]; }
};

// Rows [16 g, 16 g + 16) of the network: S recurrent steps, LayerNorm, activation, feed-forward head.  The workgroup has
// H / 16 waves and wave w owns the hidden slice [16 w, 16 w + 16) of all four gates (see lstm.hip).  STEP = false (K18):
// the outputs go to a.out.  STEP = true (K21): they stay in LDS -- the returned pointer, row stride kLFS, valid after
// the call for every thread -- for the one-lane-per-row heads; the final (h, c) also go to a.hn_row / a.cn_row, and
// a.hn / a.cn (which may be a.h0 / a.c0: a workgroup reads only its own 16 rows, all of them before its first barrier,
// and writes them after its last recurrent step) are written only when *a.commit says so.  XRows: where the input rows
// lie (LstmXDense / LstmXBlocks above).
template <int H, bool STEP, class XRows = LstmXDense>
__device__ __forceinline__ const float* lstm_rows_forward(const LstmArgs& a, const int g_tile, const XRows xrows = XRows()) {
    constexpr int HT = H / 16, NT = HT * 64, HS = H + 4, XS = kLMaxIn + 4;
    static_assert(2 * kLRows * XS >= kLRows * HS + 2 * kLRows * kLFS, "head buffers reuse the x buffers");
    __shared__ float xs[2 * kLRows * XS];
    __shared__ float hs[2][kLRows * HS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = (long)g_tile * kLRows;
    const long N = a.N;
    const int S = a.S, I = a.I, Ip = (a.I + 15) & ~15;
    const int j = 16 * w + (lane & 15);
    const float* Wih = a.P + a.L.w_ih;
    const float* Whh = a.P + a.L.w_hh;

    // H <= 64: the four gate blocks stay in VGPRs for the window; H = 128 (128 VGPRs of them, more than the 256-register
    // budget of 8 waves per CU leaves beside the rest) re-reads one gate block at a time from the L1 / L2 every step
    constexpr bool kResident = H <= 64;
    float4 fr[kResident ? 4 : 1][HT];
    if constexpr (kResident) {
#pragma unroll
        for (int q = 0; q < 4; ++q) load_fwd_frags<HT>(Whh, q * H + 16 * w, lane, fr[q]);
    }
    float bias[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bias[q] = a.P[a.L.b_ih + q * H + j] + a.P[a.L.b_hh + q * H + j];

    auto load_x = [&](int t, float* dst) {
        for (int e = tid; e < kLRows * Ip; e += NT) {
            const int r = e / Ip, k = e - r * Ip;
            const long n = r0 + r;
            dst[r * XS + k] = (n < N && k < I) ? xrows.load(a, n, S, t, I, k) : 0.f;
        }
    };
    for (int e = tid; e < kLRows * H; e += NT) {
        const int r = e / H, k = e - r * H;
        const long n = r0 + r;
        hs[0][r * HS + k] = n < N ? a.h0[n * H + k] : 0.f;
    }
    float cr[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const long n = r0 + 4 * (lane >> 4) + g;
        cr[g] = n < N ? a.c0[n * H + j] : 0.f;
    }
    load_x(0, xs);
    __syncthreads();

    for (int t = 0; t < S; ++t) {
        const float* xb = xs + (t & 1) * kLRows * XS;
        const float* hb = hs[t & 1];
        f32x4 z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (!kResident) load_fwd_frags<HT>(Whh, q * H + 16 * w, lane, fr[0]);
            f32x4 acc = {bias[q], bias[q], bias[q], bias[q]};
            const float* wr = Wih + (long)(q * H + j) * I;
#pragma unroll 1
            for (int c = 0; c < Ip / 16; ++c) {
                const int k0 = 16 * c + 4 * (lane >> 4);
                const float4 x4 = *reinterpret_cast<const float4*>(xb + (lane & 15) * XS + k0);
                const float b0 = k0 < I ? wr[k0] : 0.f, b1 = k0 + 1 < I ? wr[k0 + 1] : 0.f;
                const float b2 = k0 + 2 < I ? wr[k0 + 2] : 0.f, b3 = k0 + 3 < I ? wr[k0 + 3] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.x, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.y, b1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.z, b2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x4.w, b3, acc, 0, 0, 0);
            }
            z[q] = acc + mfma_rows_x_frags<HT>(hb, HS, lane, fr[kResident ? q : 0], 0.f);
        }
        float* hnext = hs[(t + 1) & 1];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rr = 4 * (lane >> 4) + g;
            const long n = r0 + rr;
            const float ig = sigm(z[0][g]), fg = sigm(z[1][g]), gg = tanhf(z[2][g]), og = sigm(z[3][g]);
            const float c = fg * cr[g] + ig * gg;
            const float h = og * tanhf(c);
            cr[g] = c;
            hnext[rr * HS + j] = h;
            if (a.stash && n < N) {
                float* gp = a.ws + a.L.gates + (n * S + t) * 4 * H + j;
                gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
                a.ws[a.L.cst + (n * S + t) * H + j] = c;
                a.ws[a.L.hst + (n * S + t) * H + j] = h;
            }
        }
        if (t + 1 < S) load_x(t + 1, xs + ((t + 1) & 1) * kLRows * XS);
        __syncthreads();
    }
    const float* hfin = hs[S & 1];
    bool keep = true;
    if constexpr (STEP) keep = a.commit == nullptr || *a.commit != 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int rr = 4 * (lane >> 4) + g;
        const long n = r0 + rr;
        if (n < N) {
            if (a.hn && keep) a.hn[n * H + j] = hfin[rr * HS + j];
            if (a.cn && keep) a.cn[n * H + j] = cr[g];
            if constexpr (STEP) {
                if (a.hn_row) a.hn_row[n * H + j] = hfin[rr * HS + j];
                if (a.cn_row) a.cn_row[n * H + j] = cr[g];
            }
        }
    }

    // ---- head: LayerNorm(H) -> activation -> Linear layers (the x buffers are free now)
    float* A0 = xs;
    float* A1 = xs + kLRows * HS;
    float* A2 = A1 + kLRows * kLFS;
    for (int r = w; r < kLRows; r += HT) {
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
        const float* W = a.P + a.L.fw[l];
        const float* b = a.P + a.L.fb[l];
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
                if (a.stash && n < N) a.ws[a.L.acts[l + 1] + n * M + m] = s;
            }
        }
        __syncthreads();
        in = ob; IS = kLFS; K = M;
    }
    return in;
}

// The backward of rows [16 g, 16 g + 16) through the head, LayerNorm and time (dgrad / BPTT): d out (a.dout) -> the
// pre-activation gradients of every Linear, of the LayerNorm output and of every (row, step)'s gates, into the
// workspace the forward stashed into.  K18's kernel (lstm.hip) and K22's fwd_bwd launch (lstm_update.hip) both
// instantiate it, so both form the same sums in the same order.
template <int H>
__device__ __forceinline__ void lstm_rows_backward(const LstmArgs& a, const int g_tile) {
    constexpr int HT = H / 16, NT = HT * 64, HS = H + 4, GS = 4 * H + 4;
    constexpr int kLds = 2 * kLRows * GS > 2 * kLRows * kLFS + kLRows * HS ? 2 * kLRows * GS : 2 * kLRows * kLFS + kLRows * HS;
    __shared__ float lds[kLds];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = (long)g_tile * kLRows;
    const long N = a.N;
    const int S = a.S, F = a.F, D = a.D, O = a.O;
    const int j = 16 * w + (lane & 15);
    float* ws = a.ws;

    // ---- head: d logits -> d pre-activation of every Linear -> d LayerNorm output -> d h_S
    float* Bc = lds;
    float* Bn = lds + kLRows * kLFS;
    float* DH = lds + 2 * kLRows * kLFS;
    for (int e = tid; e < kLRows * O; e += NT) {
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
        for (int e = tid; e < kLRows * K; e += NT) {
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
    for (int r = w; r < kLRows; r += HT) {
        const long n = r0 + r;
        if (n >= N) {
            for (int k = lane; k < H; k += 64) DH[r * HS + k] = 0.f;
            continue;
        }
        const float mean = ws[a.L.stats + 2 * n], rstd = ws[a.L.stats + 2 * n + 1];
        const float* hS = ws + a.L.hst + (n * S + S - 1) * H;
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
    // W_hh^T slice of this wave: B[k][col] = W_hh[k][16 w + col], k over the 4H gate rows
    float4 fr[4 * HT];
    {
        const float* Whh = a.P + a.L.w_hh + (long)(4 * (lane >> 4)) * H + j;
#pragma unroll
        for (int c = 0; c < 4 * HT; ++c) {
            const float* wp = Whh + (long)(16 * c) * H;
            fr[c] = make_float4(wp[0], wp[H], wp[2 * H], wp[3 * H]);
        }
    }
    __syncthreads();                                          // DH shares the LDS with the dgates buffers

    for (int t = S - 1; t >= 0; --t) {
        float* gb = lds + (t & 1) * kLRows * GS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rr = 4 * (lane >> 4) + g;
            const long n = r0 + rr;
            float dai = 0.f, daf = 0.f, dag = 0.f, dao = 0.f;
            if (n < N) {
                const float* gp = ws + a.L.gates + (n * S + t) * 4 * H + j;
                const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
                const float ct = ws[a.L.cst + (n * S + t) * H + j];
                const float cp = t > 0 ? ws[a.L.cst + (n * S + t - 1) * H + j] : a.c0[n * H + j];
                const float tc = tanhf(ct);
                const float dcv = dc[g] + dh[g] * og * (1.f - tc * tc);
                dai = dcv * gg * (ig * (1.f - ig));
                daf = dcv * cp * (fg * (1.f - fg));
                dag = dcv * ig * (1.f - gg * gg);
                dao = dh[g] * tc * (og * (1.f - og));
                dc[g] = dcv * fg;
                float* dp = ws + a.L.dG + (n * S + t) * 4 * H + j;
                dp[0] = dai; dp[H] = daf; dp[2 * H] = dag; dp[3 * H] = dao;
            }
            gb[rr * GS + j] = dai; gb[rr * GS + H + j] = daf; gb[rr * GS + 2 * H + j] = dag; gb[rr * GS + 3 * H + j] = dao;
        }
        __syncthreads();
        if (t > 0) {
            const f32x4 acc = mfma_rows_x_frags<4 * HT>(gb, GS, lane, fr, 0.f);
#pragma unroll
            for (int g = 0; g < 4; ++g) dh[g] = acc[g];
        }
    }
}

// ---- weight gradients: out[i][j] (+)= sum over samples s of A[s][i] * B(s, j)
enum { kBDense = 0, kBOnes = 1, kBHPrev = 2, kBDiag = 3 };
struct WJob {
    const float* A;
    const float* B;
    const float* B0;          // kBHPrev: h0 [N, ldb] (the previous state of step 0)
    float* out;
    float* out2;              // second destination (b_ih and b_hh receive the same gradient)
    long K;                   // samples
    int lda, ldb, M, Nc, ldo, mode, S, tiles_n, tile_begin;
};
struct WJobs {
    WJob j[kLMaxJobs];
    int n;
};

// One 16 x 16 output tile of a job, by a workgroup of 256 threads: four waves reduce over the samples in a fixed order
// and are added in wave order.  ADD (K18): the tile is added to the gradient bucket; otherwise (K22) it is stored, so
// that nothing has to clear the bucket first.  Returns the element this thread wrote (0 for a thread that wrote none):
// K22 forms the clip norm from it.
template <bool ADD>
__device__ __forceinline__ float lstm_wgrad_tile(const WJob& jb, const int tile, float (*part)[64][4]) {
    const int i0 = (tile / jb.tiles_n) * 16, j0 = (tile % jb.tiles_n) * 16;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long K = jb.K;
    if (jb.mode == kBDiag) {
        const int jc = j0 + (lane & 15), s4 = lane >> 4;
        float p = 0.f;
        if (jc < jb.Nc)
            for (long s = 4 * w + s4; s < K; s += 16) p += jb.A[s * jb.lda + jc] * (jb.B ? jb.B[s * jb.ldb + jc] : 1.f);
        part[w][lane][0] = p;
        __syncthreads();
        if (tid < 16 && j0 + tid < jb.Nc) {
            float v = 0.f;
            for (int ww = 0; ww < 4; ++ww)
                for (int q = 0; q < 4; ++q) v += part[ww][16 * q + tid][0];
            if constexpr (ADD) jb.out[j0 + tid] += v; else jb.out[j0 + tid] = v;
            return v;
        }
        return 0.f;
    }
    const int i = i0 + (lane & 15), jc = j0 + (lane & 15), s4 = lane >> 4;
    const bool iok = i < jb.M, jok = jc < jb.Nc;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long base = 16 * w; base < K; base += 64) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long s = base + 4 * s4 + u;
            float av = 0.f, bv = 0.f;
            if (s < K) {
                if (iok) av = jb.A[s * jb.lda + i];
                if (jb.mode == kBDense) {
                    if (jok) bv = jb.B[s * jb.ldb + jc];
                } else if (jb.mode == kBOnes) {
                    bv = jc == 0 ? 1.f : 0.f;
                } else if (jok) {                                   // kBHPrev
                    const long t = s % jb.S;
                    bv = t > 0 ? jb.B[(s - 1) * jb.ldb + jc] : jb.B0[(s / jb.S) * jb.ldb + jc];
                }
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) part[w][lane][g] = acc[g];
    __syncthreads();
    const int ln = tid >> 2, g = tid & 3;
    const float v = part[0][ln][g] + part[1][ln][g] + part[2][ln][g] + part[3][ln][g];
    const int row = i0 + 4 * (ln >> 4) + g, col = j0 + (ln & 15);
    if (row < jb.M && col < jb.Nc) {
        if constexpr (ADD) {
            jb.out[(long)row * jb.ldo + col] += v;
            if (jb.out2) jb.out2[(long)row * jb.ldo + col] += v;
        } else {
            jb.out[(long)row * jb.ldo + col] = v;
            if (jb.out2) jb.out2[(long)row * jb.ldo + col] = v;
        }
        return v;
    }
    return 0.f;
}


// host: the weight-gradient jobs of one network (a.N rows of a.S steps; x [N, S, I] and h0 [N, H] are what its forward
// read, G its gradient bucket) appended to jobs[n..]; tiles are numbered from tile_begin.  Returns the tile count after them.
inline int lstm_wgrad_add_jobs(WJob* jobs, int& n, int tile_begin, const LstmArgs& a, const int H, const float* x, const float* h0,
                               float* G) {
    const LstmLayout& L = a.L;
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
    add(ws + L.dG, 4 * H, x, I, nullptr, 4 * H, I, kBDense, NS, G + L.w_ih, nullptr, I);
    add(ws + L.dG, 4 * H, ws + L.hst, H, h0, 4 * H, H, kBHPrev, NS, G + L.w_hh, nullptr, H);
    add(ws + L.dG, 4 * H, nullptr, 0, nullptr, 4 * H, 1, kBOnes, NS, G + L.b_ih, G + L.b_hh, 1);
    add(ws + L.dy, H, ws + L.xhat, H, nullptr, 1, H, kBDiag, N, G + L.ln_w, nullptr, 1);
    add(ws + L.dy, H, nullptr, H, nullptr, 1, H, kBDiag, N, G + L.ln_b, nullptr, 1);
    for (int l = 0; l <= D; ++l) {
        const int M = l == D ? O : F, K = l == 0 ? H : F;
        add(ws + L.dz[l], M, ws + L.acts[l], K, nullptr, M, K, kBDense, N, G + L.fw[l], nullptr, K);
        add(ws + L.dz[l], M, nullptr, 0, nullptr, M, 1, kBOnes, N, G + L.fb[l], nullptr, 1);
    }
    return nt;
}


}  // namespace ppoaf
