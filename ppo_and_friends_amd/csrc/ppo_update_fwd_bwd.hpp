// K12's fwd_bwd launch: the two kernels (one workgroup per 16-row tile; 256-wide networks' tiles on workgroup pairs) and
// their launchers, shared by the translation units that instantiate them -- ppo_update.hip (pairs of equal widths, 128/256,
// 64/128), ppo_update_lean.hip (the lean kernel of the epoch driver's case, below), ppo_update_narrow.hip (the narrow-actor pairs 64/256, 32/256, 32/64) and ppo_update_wide.hip (256/512, whose
// critic runs the body of ppo_update_rowtile_wide.hpp): one hipcc process each, so that none is the build's long pole alone.  Which unit holds which pair: PPOAF_WIDTH_PAIRS, ppo_update_dev.hpp.
#pragma once
#include "ppo_update_rowpair.hpp"
#include <hip/hip_ext.h>

namespace ppoaf {

// 1-D grid of 2 * n_wg workgroups.  Every workgroup of a network streams that network's whole
// weight set, so workgroups of one network are placed on the same XCDs (blocks b and b + 8 share
// an XCD under the observed round-robin dispatch): XCDs 0-3 take the actor, 4-7 the critic, and
// each weight line is then fetched into an XCD's L2 once for its 4 consumers instead of once per
// pair.  Placement only changes speed; nothing depends on it.
template <int HTA, int HTC, bool SPLIT>
__global__ __launch_bounds__(kThreadsU) void ppo_update_fwd_bwd_kernel(UpdateDev u) {
    const int b = rowtile_request_args(u, blockIdx.x);     // one round trip for the argument block, then the cursor's
    int which = (b >> 2) & 1;                              // b % 8 in {0..3} -> actor, {4..7} -> critic
    int g = ((b >> 3) << 2) | (b & 3);
    if (u.confine) {                                // one half of the XCDs left to another chain (args->xcd_half)
        const int x = b & 7;
        if ((x >> 2) != u.confine - 1) return;
        which = (x & 3) >> 1;                              // the half's first two XCDs: actor, the other two: critic
        g = ((b >> 3) << 1) | (x & 1);
    }
    if (g >= u.n_wg) return;                               // uniform per workgroup, before any barrier
    // (a wide pair's kernel alone reads the layer-0 panel's row stride from its arguments: u.sp.xld, PPOAF_SPLIT_WIDE_INPUTS / _SHAPES)
    constexpr bool XLD = SPLIT && HTC > 16;
    if (which == 0) ppo_update_fwd_bwd_body<HTA, SPLIT, XLD>(u, 0, g);
    else ppo_update_fwd_bwd_body<HTC, SPLIT, XLD>(u, 1, g);
}

// args->row_pairs (split-wgrad chain): a 256-wide network's row tiles on pairs of workgroups (ppo_update_rowpair.hpp); the
// other network's tiles as above.  Workgroup b runs on XCD b % 8; slot j = b / 8 of an XCD holds tile pair member j & 1.
template <int HTA, int HTC>
__global__ __launch_bounds__(kThreadsU) void ppo_update_fwd_bwd_pair_kernel(UpdateDev u, PairDev pd) {
    const int b = blockIdx.x, x = b & 7, j = b >> 3;
    int which, g, hf = 0;
    if (u.confine) {
        if ((x >> 2) != u.confine - 1) return;
        which = (x & 3) >> 1;
        if (which == 0 ? HTA == 16 : HTC == 16) { hf = j & 1; g = ((j >> 1) << 1) | (x & 1); }
        else g = (j << 1) | (x & 1);
    } else {
        which = x >> 2;
        if (which == 0 ? HTA == 16 : HTC == 16) { hf = j & 1; g = ((j >> 1) << 2) | (x & 3); }
        else g = (j << 2) | (x & 3);
    }
    if (g >= u.n_wg) return;                               // uniform per workgroup, before any barrier
    if (which == 0) {
        if constexpr (HTA == 16) ppo_update_fwd_bwd_pair_body<16>(u, 0, g, hf, pd);
        else ppo_update_fwd_bwd_body_as<HTA, true, false>(u, 0, g);     // (the 256-wide partner's pairs set this launch's time)
    } else {
        if constexpr (HTC == 16) ppo_update_fwd_bwd_pair_body<16>(u, 1, g, hf, pd);
        else ppo_update_fwd_bwd_body_as<HTC, true, false>(u, 1, g);
    }
}

template <int HTA, int HTC, bool SPLIT>
inline int launch_fwd_bwd_as(const UpdateDev& u, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_update_fwd_bwd_kernel<HTA, HTC, SPLIT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = u.confine ? 8u * (unsigned)((u.n_wg + 1) / 2) : 8u * (unsigned)((u.n_wg + 3) / 4);     // groups of 4 actor + 4 critic blocks
    if (e0 || e1)        // the kernel's own begin / end stamped into the events (bench.py: roofline_update)
        hipExtLaunchKernelGGL((ppo_update_fwd_bwd_kernel<HTA, HTC, SPLIT>), dim3(grid), dim3(kThreadsU), lds, s, e0, e1, 0, u);
    else
        hipLaunchKernelGGL((ppo_update_fwd_bwd_kernel<HTA, HTC, SPLIT>), dim3(grid), dim3(kThreadsU), lds, s, u);
    return check_launch("ppo_update_fwd_bwd");
}

// split-wgrad chain with args->row_pairs: the 256-wide networks' tiles on workgroup pairs
template <int HTA, int HTC>
inline int launch_fwd_bwd_pairs(const UpdateDev& u, const PairDev& pd, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ppo_update_fwd_bwd_pair_kernel<HTA, HTC>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    // slots per XCD: two per tile of a paired network (both networks share the grid: the wider need decides)
    const unsigned per_slot = u.confine ? 2u : 4u;
    const unsigned grid = 8u * 2u * (unsigned)((u.n_wg + per_slot - 1) / per_slot);
    if (e0 || e1)
        hipExtLaunchKernelGGL((ppo_update_fwd_bwd_pair_kernel<HTA, HTC>), dim3(grid), dim3(kThreadsU), lds, s, e0, e1, 0, u, pd);
    else
        hipLaunchKernelGGL((ppo_update_fwd_bwd_pair_kernel<HTA, HTC>), dim3(grid), dim3(kThreadsU), lds, s, u, pd);
    return check_launch("ppo_update_fwd_bwd(row pairs)");
}

// the pair kernel of width pair <HA, HC>: only pairs with a 256-wide critic have one (pairs_run)
template <int HA, int HC>
inline int launch_fwd_bwd_pairs_of(const UpdateDev& u, const PairDev& pd, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if constexpr (HC == 256) return launch_fwd_bwd_pairs<HA / 16, 16>(u, pd, lds, s, e0, e1);
    set_error("ppo_update_fwd_bwd(row pairs): no pair kernel for hidden widths (actor %d, critic %d)", HA, HC);
    return PPOAF_E_INVALID;
}

template <int HTA, int HTC>
inline int launch_fwd_bwd(const UpdateDev& u, size_t lds, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    return u.split ? launch_fwd_bwd_as<HTA, HTC, true>(u, lds, s, e0, e1) : launch_fwd_bwd_as<HTA, HTC, false>(u, lds, s, e0, e1);
}

// one rung of the dispatch: the launch of width pair <HA, HC> for these args
struct FwdBwdLaunch {
    const UpdateDev& u; const ppoaf_ppo_update_args_t* args; size_t lds; hipStream_t s; hipEvent_t e0, e1;
};
// The lean kernel (ppo_update_lean.hip): the row-tile body compiled for one (activation, head), split-wgrad chain and
// per-epoch-tables flavour only.  fwd_bwd_lean_form evaluates ONCE per launch, on the host, what ppo_update_fwd_bwd_body asks in
// every workgroup (depth 3 on both networks, tables in batch order, no row_map), and: the split-wgrad chain, one activation code
// for both networks, a Categorical or Gaussian head, a width pair with an instantiation (32/32, 64/64, 128/128, 64/128).
bool fwd_bwd_lean_form(const UpdateDev& u);
int fwd_bwd_launch_lean(const FwdBwdLaunch& L);

template <int HA, int HC>
inline int fwd_bwd_launch_pair(const FwdBwdLaunch& L) {
    const UpdateDev& u = L.u;
    if (u.split && args_row_pairs(L.args) && pairs_run(u.net[0], u.net[1])) {
        PairDev pd;
        pair_region_layout(u, &pd, reinterpret_cast<char*>(L.args->split_workspace) + pair_region_offset(u));
        return launch_fwd_bwd_pairs_of<HA, HC>(u, pd, L.lds, L.s, L.e0, L.e1);
    }
    if (fwd_bwd_lean_form(u)) return fwd_bwd_launch_lean(L);
    // other shapes (a 256-wide network of depth 1 or > 4): one workgroup per tile
    return launch_fwd_bwd<HA / 16, HC / 16>(u, L.lds, L.s, L.e0, L.e1);
}
// the narrow-actor pairs' rungs, then the refusal of a pair the list does not name (ppo_update_narrow.hip)
int fwd_bwd_launch_narrow(const FwdBwdLaunch& L);
// the wide pairs' rungs (ppo_update_wide.hip): the split-wgrad chain only, one workgroup per tile
int fwd_bwd_launch_wide(const FwdBwdLaunch& L);
// ... with more than 8 actor outputs (ppo_update_wide_heads.hip: the wide heads, a kernel of their own)
int fwd_bwd_launch_wide_heads(const FwdBwdLaunch& L);

}  // namespace ppoaf
