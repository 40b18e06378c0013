// K12's fwd_bwd launch for what the epoch driver of fused_update.py runs: the lean row-tile kernel.
//
// ppo_update_fwd_bwd_kernel<HTA, HTC, SPLIT> holds two flavours of the row-tile body per network (TABLES and not), chosen per
// workgroup from the arguments, and inside either every activation and every head, chosen per use.  None of that changes
// during a training run.  The kernel here is compiled for ONE case: the split-wgrad chain, the per-epoch-tables flavour
// (three hidden layers, tables in batch order, no row_map), one activation code for both networks and one head kind -- the
// same body (ppo_update_rowtile.hpp) with those as template parameters, so the same expressions in the same order: results
// are bitwise those of the general kernel.  The host evaluates the conditions once per launch (fwd_bwd_lean_form) and
// launches this kernel when all of them hold; every other case keeps the general kernel.  Block -> (network, tile) mapping,
// `confine`, LDS size, grid and block size are the general kernel's.  A translation unit of its own: one hipcc process.
#include "ppo_update_fwd_bwd.hpp"

namespace ppoaf {

template <int HTA, int HTC, int ACT, int HEAD>
__global__ __launch_bounds__(kThreadsU) void ppo_update_fwd_bwd_lean_kernel(UpdateDev u) {
    static_assert(HTA <= kNW && HTC <= kNW, "the per-epoch-tables flavour: one output tile per wave");
    const int b = rowtile_request_args(u, blockIdx.x);     // (as ppo_update_fwd_bwd_kernel, ppo_update_fwd_bwd.hpp)
    int which = (b >> 2) & 1;
    int g = ((b >> 3) << 2) | (b & 3);
    if (u.confine) {
        const int x = b & 7;
        if ((x >> 2) != u.confine - 1) return;
        which = (x & 3) >> 1;
        g = ((b >> 3) << 1) | (x & 1);
    }
    if (g >= u.n_wg) return;                               // uniform per workgroup, before any barrier
    // (three hidden layers: fwd_bwd_lean_form has checked it.  The general kernel's body learns it from its own run-time test
    //  ahead of this flavour and unrolls the layer loops on it; here the compiler is told.)
    __builtin_assume(u.net[0].depth == 3 && u.net[1].depth == 3);
    if (which == 0) ppo_update_fwd_bwd_body_as<HTA, true, true, false, ACT, HEAD>(u, 0, g);
    else ppo_update_fwd_bwd_body_as<HTC, true, true, false, ACT, HEAD>(u, 1, g);
}

// the width pairs, activations and heads the lean kernel is instantiated for
#define PPOAF_LEAN_PAIRS(X) X(32, 32) X(64, 64) X(128, 128) X(64, 128)
static bool lean_pair(const int ha, const int hc) {
#define PPOAF_WIDTH_PAIR_CALL_(A, C) true
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_LEAN_PAIRS, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    return false;
}

bool fwd_bwd_lean_form(const UpdateDev& u) {
    const NetDev& a = u.net[0];
    const NetDev& c = u.net[1];
    return u.split && a.depth == 3 && c.depth == 3 && u.pregathered && !u.row_map &&        // what the body asked per workgroup
           a.act == c.act && a.act >= PPOAF_ACT_RELU && a.act <= PPOAF_ACT_TANH &&
           (u.head_kind == PPOAF_HEAD_CATEGORICAL || u.head_kind == PPOAF_HEAD_GAUSSIAN) && lean_pair(a.H, c.H);
}

template <int HTA, int HTC, int ACT, int HEAD>
static int launch_lean_as(const FwdBwdLaunch& L) {
    const UpdateDev& u = L.u;
    static bool attr_set = false;
    if (!attr_set && L.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_update_fwd_bwd_lean_kernel<HTA, HTC, ACT, HEAD>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = u.confine ? 8u * (unsigned)((u.n_wg + 1) / 2) : 8u * (unsigned)((u.n_wg + 3) / 4);     // launch_fwd_bwd_as's
    if (L.e0 || L.e1)
        hipExtLaunchKernelGGL((ppo_update_fwd_bwd_lean_kernel<HTA, HTC, ACT, HEAD>), dim3(grid), dim3(kThreadsU), L.lds, L.s, L.e0, L.e1, 0, u);
    else
        hipLaunchKernelGGL((ppo_update_fwd_bwd_lean_kernel<HTA, HTC, ACT, HEAD>), dim3(grid), dim3(kThreadsU), L.lds, L.s, u);
    return check_launch("ppo_update_fwd_bwd(lean)");
}

template <int HA, int HC>
static int launch_lean_pair(const FwdBwdLaunch& L) {
    const int act = L.u.net[0].act;
    const bool gauss = L.u.head_kind == PPOAF_HEAD_GAUSSIAN;
#define PPOAF_LEAN_ACT_(ACT)                                                                                   \
    if (act == ACT) return gauss ? launch_lean_as<HA / 16, HC / 16, ACT, PPOAF_HEAD_GAUSSIAN>(L)                \
                                 : launch_lean_as<HA / 16, HC / 16, ACT, PPOAF_HEAD_CATEGORICAL>(L);
    PPOAF_LEAN_ACT_(PPOAF_ACT_RELU) PPOAF_LEAN_ACT_(PPOAF_ACT_LEAKY_RELU) PPOAF_LEAN_ACT_(PPOAF_ACT_TANH)
#undef PPOAF_LEAN_ACT_
    set_error("ppo_update_fwd_bwd(lean): no kernel for activation %d", act);
    return PPOAF_E_INVALID;
}

int fwd_bwd_launch_lean(const FwdBwdLaunch& L) {
    if (fwd_bwd_lean_form(L.u)) {
#define PPOAF_WIDTH_PAIR_CALL_(A, C) launch_lean_pair<A, C>(L)
        PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_LEAN_PAIRS, L.u.net[0].H, L.u.net[1].H)
#undef PPOAF_WIDTH_PAIR_CALL_
    }
    set_error("ppo_update_fwd_bwd(lean): these arguments do not select the lean kernel");     // a missing kernel is an error
    return PPOAF_E_INVALID;
}

}  // namespace ppoaf

#ifdef PPOAF_STAMPS
// (diagnostic build: the stamp buffers are per translation unit -- these read the lean kernel's; tools/phase_stamps.py)
extern "C" int ppoaf_debug_read_lean_stamps(unsigned long long* out /* host [32] */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ppoaf::g_ppo_update_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -2;
}
extern "C" int ppoaf_debug_read_lean_hidden_stamps(unsigned long long* out /* host [2][8][8] */) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ppoaf::g_ppo_hidden_stamps), sizeof(unsigned long long) * 128) == hipSuccess ? 0 : -2;
}
#endif
