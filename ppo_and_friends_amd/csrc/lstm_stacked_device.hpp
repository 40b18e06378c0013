// What the two-layer LSTM kernels share: K18 for two stacked layers (lstm_stacked.hip) and the one-launch rollout /
// evaluation step of such a pair (lstm_stacked_step.hip).  Descriptor check, bucket and workspace layout, kernel
// arguments, the streamed fragment loaders and the cell update -- one copy of each, so a step of the one-launch kernel
// and a one-step call of ppoaf_lstm2_forward run the same cell code on the same sums.
#pragma once
#include "lstm_device.hpp"

namespace ppoaf {
namespace {

#define PPOAF_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

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

}  // namespace
}  // namespace ppoaf
