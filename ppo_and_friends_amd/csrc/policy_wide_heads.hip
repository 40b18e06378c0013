// K6+K7 and K19 for the wide heads of the 256/512 pair: a 256-wide actor with 9 .. 24 outputs (kWideOut), Categorical or
// tanh-Gaussian -- humanoid's Box(17), mario_bros_ram's Discrete(18).  The bodies are the ones of policy_step.hip and
// policy_infer.hip (policy_rows.hpp) with the output carve and the Categorical row 24 wide (KO = kWideOut): sWout holds
// [24, H], a row of sOut 24 floats, the per-class registers 24 values indexed by unrolled loop counters only.  Classes and
// dimensions 0 .. 7 take the operations of the narrow kernels in their order, and the Philox counters are theirs: a row draws
// (seed, offset + e, 0).x (Discrete) or the blocks (seed, offset + e, d / 4) (Box).  Kernels of their own, in a translation
// unit of their own: a launch with out_dim <= 8 runs the kernel it always ran.
#include "policy_rows.hpp"

namespace ppoaf {

template <int HTA, int HTC>
__global__ __launch_bounds__(kThreadsS) void policy_step_wide_heads_kernel(StepDev u) {
    const int b = blockIdx.x;
    const int which = (b >> 2) & 1;
    const int g = ((b >> 3) << 2) | (b & 3);
    if (g >= u.n_wg) return;
    if (which == 0) policy_step_body<HTA, false, false, kWideOut>(u, 0, g);
    else policy_step_body<HTC, false>(u, 1, g);
}

template <int HTA, int HTC>
__global__ __launch_bounds__(kThreadsS) void policy_step_blocks_wide_heads_kernel(StepDev u, StepBlocks tb) {
    const int b = blockIdx.x;
    const int which = (b >> 2) & 1;
    const int g = ((b >> 3) << 2) | (b & 3);
    if (g >= u.n_wg) return;
    if (which == 0) policy_step_body<HTA, false, true, kWideOut>(u, 0, g, &tb);
    else policy_step_body<HTC, false, true>(u, 1, g, &tb);
}

// K19 (policy_infer_kernel, policy_infer.hip) with the 24-wide carve: the forward, then the Categorical or Gaussian row
template <int HT>
__global__ __launch_bounds__(kThreadsU) void policy_infer_wide_heads_kernel(InferDev u) {
    constexpr int OS = mlp_rows_out_stride(kWideOut);
    const int tid = threadIdx.x;
    const NetDev& nd = u.net;
    const int out_dim = nd.out_dim;
    const long e0 = (long)blockIdx.x * kRows;
    const float* sOut = mlp_rows_forward<HT, void, kWideOut>(nd, u.params, u.obs, nullptr, u.E, e0,
                                                            reinterpret_cast<float*>(policy_infer_smem));
    // heads: one lane per env row
    if (tid >= kRows || e0 + tid >= u.E) return;
    const float* zr = sOut + tid * OS;
    const long e = e0 + tid;
    const bool greedy = u.mode == PPOAF_INFER_DETERMINISTIC;
    if (u.head_kind == PPOAF_HEAD_CATEGORICAL)
        cat_infer_row<kWideOut>(zr, out_dim, greedy, e, u.seed, u.offset, u.action_out);
    else
        gauss_infer_row(zr, out_dim, greedy, u.params + nd.offset + nd.log_std_off, u.min_std, u.act_lo, u.act_hi, e,
                        u.seed, u.offset, u.action_out);
}

// dynamic LDS beyond 64 KB is asked for once per kernel
template <class Kernel>
static int allow_lds(Kernel k, bool& done, size_t lds) {
    if (!done && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        done = true;
    }
    return PPOAF_OK;
}

template <int HA, int HC>
static int launch_step_pair(const StepDev& u, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    const int rc = allow_lds(policy_step_wide_heads_kernel<HA / 16, HC / 16>, attr_set, lds);
    if (rc) return rc;
    const unsigned grid = 8u * (unsigned)((u.n_wg + 3) / 4);
    hipLaunchKernelGGL((policy_step_wide_heads_kernel<HA / 16, HC / 16>), dim3(grid), dim3(kThreadsS), lds, s, u);
    return check_launch("policy_step");
}

template <int HA, int HC>
static int launch_step_blocks_pair(const StepDev& u, const StepBlocks& tb, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    const int rc = allow_lds(policy_step_blocks_wide_heads_kernel<HA / 16, HC / 16>, attr_set, lds);
    if (rc) return rc;
    const unsigned grid = 8u * (unsigned)((u.n_wg + 3) / 4);
    hipLaunchKernelGGL((policy_step_blocks_wide_heads_kernel<HA / 16, HC / 16>), dim3(grid), dim3(kThreadsS), lds, s, u, tb);
    return check_launch("policy_step_blocks");
}

int launch_step_wide_heads(const StepDev& u, size_t lds, hipStream_t s) {
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) launch_step_pair<A, C>(u, lds, s)
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_WIDE, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("policy_step: hidden widths (actor %d, critic %d) have no wide heads (out_dim %d)", ha, hc, u.net[0].out_dim);
    return PPOAF_E_INVALID;
}

int launch_step_blocks_wide_heads(const StepDev& u, const StepBlocks& tb, size_t lds, hipStream_t s) {
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) launch_step_blocks_pair<A, C>(u, tb, lds, s)
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_WIDE, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("policy_step_blocks: hidden widths (actor %d, critic %d) have no wide heads (out_dim %d)", ha, hc, u.net[0].out_dim);
    return PPOAF_E_INVALID;
}

int launch_infer_wide_heads(const InferDev& u, size_t lds, hipStream_t s) {
    if (u.net.H != 256) {
        set_error("policy_infer: hidden width %d has no wide heads (out_dim %d)", u.net.H, u.net.out_dim);
        return PPOAF_E_INVALID;
    }
    static bool attr_set = false;
    const int rc = allow_lds(policy_infer_wide_heads_kernel<16>, attr_set, lds);
    if (rc) return rc;
    const unsigned grid = (unsigned)((u.E + kRows - 1) / kRows);
    hipLaunchKernelGGL((policy_infer_wide_heads_kernel<16>), dim3(grid), dim3(kThreadsU), lds, s, u);
    return check_launch("policy_infer");
}

}  // namespace ppoaf
