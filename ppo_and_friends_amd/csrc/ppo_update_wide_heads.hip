// K12's fwd_bwd kernel for the wide heads of the wide width pair (256, 512): a 256-wide actor with 9 .. 24 outputs
// (Categorical or tanh-Gaussian), whose tiles run the body of ppo_update_rowtile_heads.hpp, beside the 512-wide critic,
// whose tiles run the body of ppo_update_rowtile_wide.hpp as they do in ppo_update_wide.hip's kernel.  A kernel of its own in
// a translation unit of its own: a launch with out_dim <= 8 runs ppo_update_fwd_bwd_kernel<16, 32, true> as before.  The
// chain ends in the wgrad and Adam launches, which take the output segment by its length.
#include "ppo_update_rowtile_wide.hpp"       // (ahead of the kernel template: it declares the critic body's specialisation)
#include "ppo_update_rowtile_heads.hpp"
#include "ppo_update_fwd_bwd.hpp"

namespace ppoaf {

// the grid and the placement of ppo_update_fwd_bwd_kernel (ppo_update_fwd_bwd.hpp)
template <int HTA, int HTC>
__global__ __launch_bounds__(kThreadsU) void ppo_update_fwd_bwd_wide_heads_kernel(UpdateDev u) {
    const int b = rowtile_request_args(u, blockIdx.x);
    int which = (b >> 2) & 1;
    int g = ((b >> 3) << 2) | (b & 3);
    if (u.confine) {
        const int x = b & 7;
        if ((x >> 2) != u.confine - 1) return;
        which = (x & 3) >> 1;
        g = ((b >> 3) << 1) | (x & 1);
    }
    if (g >= u.n_wg) return;                               // uniform per workgroup, before any barrier
    if (which == 0) ppo_update_fwd_bwd_body_heads<HTA>(u, g);
    else ppo_update_fwd_bwd_body<HTC, true, true>(u, 1, g);
}

template <int HA, int HC>
static int fwd_bwd_launch_wide_heads_pair(const FwdBwdLaunch& L) {
    static_assert(HC / 16 == kWideHT, "the wide body is the 512-wide critic's");
    const UpdateDev& u = L.u;
    static bool attr_set = false;
    if (!attr_set && L.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_update_fwd_bwd_wide_heads_kernel<HA / 16, HC / 16>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = u.confine ? 8u * (unsigned)((u.n_wg + 1) / 2) : 8u * (unsigned)((u.n_wg + 3) / 4);
    if (L.e0 || L.e1)
        hipExtLaunchKernelGGL((ppo_update_fwd_bwd_wide_heads_kernel<HA / 16, HC / 16>), dim3(grid), dim3(kThreadsU), L.lds, L.s,
                              L.e0, L.e1, 0, u);
    else
        hipLaunchKernelGGL((ppo_update_fwd_bwd_wide_heads_kernel<HA / 16, HC / 16>), dim3(grid), dim3(kThreadsU), L.lds, L.s, u);
    return check_launch("ppo_update_fwd_bwd");
}

int fwd_bwd_launch_wide_heads(const FwdBwdLaunch& L) {
    const int ha = L.u.net[0].H, hc = L.u.net[1].H;
    PPOAF_REQUIRE(L.u.split, "ppo_update_fwd_bwd: the wide pair (actor %d, critic %d) has no slab form: args->split_workspace is not set",
                  ha, hc);
#define PPOAF_WIDTH_PAIR_CALL_(A, C) fwd_bwd_launch_wide_heads_pair<A, C>(L)
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_WIDE, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("ppo_update_fwd_bwd: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

}  // namespace ppoaf
