// K18 at hidden width 256: the forward and backward kernels of the one-layer LSTM network of LSTMNetwork.forward_logits
// (networks/ppo_networks/lstm.py:103-127) for the width lstm.hip's H / 16-waves-per-16-rows scheme does not reach (16 waves
// of 128 registers, and a W_hh of 1 MiB).  Rows are split into tiles of 32 (two MFMA M tiles) per workgroup of 8 waves;
// wave w owns the hidden units [32 w, 32 w + 32) of all four gates, so the cell update stays lane-local and only h
// (forward, double-buffered) and a step's d gates (backward) cross waves through LDS.  W_hh is streamed from the L2 every
// step as whole 128-byte lines, requested a tile ahead of the MFMAs that consume it, and every fragment feeds both M
// tiles (lstm_wide_device.hpp).  Sums run in a fixed order: bitwise reproducible, no atomics.  The weight gradients are
// lstm.hip's launch (lstm_wgrad_tile is generic in H); the entry points are lstm.hip's too.
#include "lstm_wide_device.hpp"

namespace ppoaf {
namespace {

extern __shared__ __attribute__((aligned(16))) unsigned char lstm_wide_smem[];

__global__ __launch_bounds__(kWThreads) void lstm_wide_fwd_kernel(const LstmArgs a) {
    lstm_wide_rows_forward<false>(a, blockIdx.x, reinterpret_cast<float*>(lstm_wide_smem));
}

__global__ __launch_bounds__(kWThreads) void lstm_wide_bwd_kernel(const LstmArgs a) {
    lstm_wide_rows_backward(a, blockIdx.x, reinterpret_cast<float*>(lstm_wide_smem));
}

}  // namespace

int lstm_wide_forward(const LstmArgs& a, hipStream_t stream) {
    static bool raised = false;
    constexpr size_t lds = kWFwdLds * sizeof(float);
    if (int rc = allow_large_lds(lstm_wide_fwd_kernel, lds, raised, "ppoaf_lstm_forward")) return rc;
    const unsigned blocks = (unsigned)((a.N + kWRows - 1) / kWRows);
    hipLaunchKernelGGL(lstm_wide_fwd_kernel, dim3(blocks), dim3(kWThreads), lds, stream, a);
    return check_launch("ppoaf_lstm_forward");
}

int lstm_wide_backward(const LstmArgs& a, hipStream_t stream) {
    static bool raised = false;
    constexpr size_t lds = kWBwdLds * sizeof(float);
    PPOAF_REQUIRE(((uintptr_t)a.ws & 7) == 0, "ppoaf_lstm_backward: the workspace must be 8-byte aligned at hidden 256");
    if (int rc = allow_large_lds(lstm_wide_bwd_kernel, lds, raised, "ppoaf_lstm_backward")) return rc;
    const unsigned blocks = (unsigned)((a.N + kWRows - 1) / kWRows);
    hipLaunchKernelGGL(lstm_wide_bwd_kernel, dim3(blocks), dim3(kWThreads), lds, stream, a);
    return check_launch("ppoaf_lstm_backward");
}

}  // namespace ppoaf
