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

// the forward body lives in lstm_device.hpp (K21, lstm_policy_step.hip, instantiates it as well), and so does the
// backward body (K22, lstm_update.hip, runs it in the launch of its forward)
template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_fwd_kernel(const LstmArgs a) {
    lstm_rows_forward<H, false>(a, blockIdx.x);
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_bwd_kernel(const LstmArgs a) {
    lstm_rows_backward<H>(a, blockIdx.x);
}

// the weight-gradient tile body lives in lstm_device.hpp as well (K22, lstm_update.hip, stores where K18 adds)
__global__ __launch_bounds__(256) void lstm_wgrad_kernel(const WJobs J) {
    __shared__ float part[4][64][4];
    int ji = 0;
    while (ji + 1 < J.n && (int)blockIdx.x >= J.j[ji + 1].tile_begin) ++ji;
    lstm_wgrad_tile<true>(J.j[ji], blockIdx.x - J.j[ji].tile_begin, part);
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
    WJobs J{};
    const int nt = lstm_wgrad_add_jobs(J.j, J.n, 0, lstm_args_of(d), d->hidden, x, h0, d->grads);
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(nt), dim3(256), 0, (hipStream_t)stream, J);
    return check_launch("ppoaf_lstm_wgrad");
}
