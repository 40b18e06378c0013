// K18: the one-layer LSTM network of LSTMNetwork.forward_logits (networks/ppo_networks/lstm.py:103-127) --
// forward (rollout step and training window), backward through the head and time (dgrad / BPTT), weight gradients.
//
// Rows are split into tiles of 16 (one MFMA M tile) per workgroup; the workgroup has H / 16 waves and wave w owns the
// hidden slice [16 w, 16 w + 16) of all four gates.  In the 16 x 16 MFMA output layout a lane then holds i, f, g, o of
// the same (row, unit) pairs, so the cell update is lane-local, and only the new h crosses waves (LDS, one barrier per
// step, double-buffered).  The wave's four W_hh gate blocks (4 x 16 rows x H) stay in VGPRs for the whole window at
// H <= 64 (H floats per lane); at H = 128 they are re-read from the L1 / L2 each step, one gate block at a time.  The backward pass keeps the transposed slice (4H x 16 columns of W_hh, again H floats per lane) and
// runs the same step structure in reverse: dgates of a step go through LDS and the MFMA forms dh_{t-1}.  The weight
// gradients are a separate launch of 16 x 16 output tiles, each reduced over (row, step) samples by four waves in a
// fixed order and summed in a fixed order: bitwise reproducible, no atomics.
#include "lstm_device.hpp"

namespace ppoaf {
namespace {

// the forward body lives in lstm_device.hpp (K21, lstm_policy_step.hip, instantiates it as well)
template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_fwd_kernel(const LstmArgs a) {
    lstm_rows_forward<H, false>(a, blockIdx.x);
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_bwd_kernel(const LstmArgs a) {
    constexpr int HT = H / 16, NT = HT * 64, HS = H + 4, GS = 4 * H + 4;
    constexpr int kLds = 2 * kLRows * GS > 2 * kLRows * kLFS + kLRows * HS ? 2 * kLRows * GS : 2 * kLRows * kLFS + kLRows * HS;
    __shared__ float lds[kLds];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long r0 = (long)blockIdx.x * kLRows;
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

__global__ __launch_bounds__(256) void lstm_wgrad_kernel(const WJobs J) {
    __shared__ float part[4][64][4];
    int ji = 0;
    while (ji + 1 < J.n && (int)blockIdx.x >= J.j[ji + 1].tile_begin) ++ji;
    const WJob& jb = J.j[ji];
    const int tile = blockIdx.x - jb.tile_begin;
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
            jb.out[j0 + tid] += v;
        }
        return;
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
        jb.out[(long)row * jb.ldo + col] += v;
        if (jb.out2) jb.out2[(long)row * jb.ldo + col] += v;
    }
}

template <template <int> class Launch, typename... T>
int dispatch_h(int H, T... args) {
    if (H == 32) return Launch<32>::run(args...);
    if (H == 64) return Launch<64>::run(args...);
    return Launch<128>::run(args...);
}

template <int H> struct FwdLaunch {
    static int run(const LstmArgs& a, hipStream_t s) {
        const unsigned blocks = (unsigned)((a.N + kLRows - 1) / kLRows);
        hipLaunchKernelGGL(lstm_fwd_kernel<H>, dim3(blocks), dim3(H / 16 * 64), 0, s, a);
        return check_launch("ppoaf_lstm_forward");
    }
};
template <int H> struct BwdLaunch {
    static int run(const LstmArgs& a, hipStream_t s) {
        const unsigned blocks = (unsigned)((a.N + kLRows - 1) / kLRows);
        hipLaunchKernelGGL(lstm_bwd_kernel<H>, dim3(blocks), dim3(H / 16 * 64), 0, s, a);
        return check_launch("ppoaf_lstm_backward");
    }
};

}  // namespace
}  // namespace ppoaf

using namespace ppoaf;

extern "C" int ppoaf_lstm_workspace_floats(const ppoaf_lstm_desc_t* d, int64_t* floats_out) {
    if (int rc = check_lstm_desc(d, false, "ppoaf_lstm_workspace_floats")) return rc;
    PPOAF_REQUIRE(floats_out != nullptr, "ppoaf_lstm_workspace_floats: floats_out is NULL");
    const LstmLayout L = layout_of(*d);
    floats_out[0] = L.total;
    floats_out[1] = L.size;
    return PPOAF_OK;
}

extern "C" int ppoaf_lstm_forward(const ppoaf_lstm_desc_t* d, const float* x, const float* h0, const float* c0,
                                  float* out, float* hn, float* cn, int32_t stash, ppoaf_stream_t stream) {
    if (int rc = check_lstm_desc(d, stash != 0, "ppoaf_lstm_forward")) return rc;
    PPOAF_REQUIRE(x && h0 && c0 && out, "ppoaf_lstm_forward: x / h0 / c0 / out is NULL");
    LstmArgs a = lstm_args_of(d);
    a.x = x; a.h0 = h0; a.c0 = c0; a.out = out; a.hn = hn; a.cn = cn; a.stash = stash != 0;
    return dispatch_h<FwdLaunch>(d->hidden, a, (hipStream_t)stream);
}

extern "C" int ppoaf_lstm_backward(const ppoaf_lstm_desc_t* d, const float* c0, const float* dout, ppoaf_stream_t stream) {
    if (int rc = check_lstm_desc(d, true, "ppoaf_lstm_backward")) return rc;
    PPOAF_REQUIRE(c0 && dout, "ppoaf_lstm_backward: c0 / dout is NULL");
    LstmArgs a = lstm_args_of(d);
    a.c0 = c0; a.dout = dout;
    return dispatch_h<BwdLaunch>(d->hidden, a, (hipStream_t)stream);
}

extern "C" int ppoaf_lstm_wgrad(const ppoaf_lstm_desc_t* d, const float* x, const float* h0, ppoaf_stream_t stream) {
    if (int rc = check_lstm_desc(d, true, "ppoaf_lstm_wgrad")) return rc;
    PPOAF_REQUIRE(x && h0 && d->grads, "ppoaf_lstm_wgrad: x / h0 / grads is NULL");
    const LstmLayout L = layout_of(*d);
    const long N = d->rows, S = d->steps, NS = N * S;
    const int I = d->in_dim, H = d->hidden, F = d->ff_hidden, D = d->ff_depth, O = d->out_dim;
    float* G = d->grads;
    const float* ws = d->workspace;
    WJobs J{};
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
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, J);
    return check_launch("ppoaf_lstm_wgrad");
}
