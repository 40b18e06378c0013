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

template <int H>
__global__ __launch_bounds__(2 * (H / 16) * 64) PPOAF_NO_PK_F32 void lstm2_forward_kernel(const Lstm2Args a) {
    lstm2_rows_forward<H, false>(a, blockIdx.x);
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) PPOAF_NO_PK_F32 void lstm2_backward_kernel(const Lstm2Args a) {
    lstm2_rows_backward<H>(a, blockIdx.x);
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
    const int nt = lstm2_wgrad_add_jobs(J.j, J.n, 0, lstm2_args_of(d), d->hidden, x, d->grads);
    hipLaunchKernelGGL(lstm2_wgrad_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, J);
    return check_launch("ppoaf_lstm2_wgrad");
}
