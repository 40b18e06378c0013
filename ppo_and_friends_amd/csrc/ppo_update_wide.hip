// K12's fwd_bwd kernel for the wide width pair (256, 512): ppo_update_fwd_bwd_kernel<16, 32, true>, whose actor tiles run
// the row-tile body of ppo_update_rowtile.hpp and whose critic tiles run the body of ppo_update_rowtile_wide.hpp.  The pair
// exists on the split-wgrad chain only and ends in the wgrad and Adam launches (PPOAF_WIDTH_PAIRS_WIDE, ppo_update_dev.hpp).
// A translation unit of its own, like ppo_update_narrow.hip: one more hipcc process of the build.
#include "ppo_update_rowtile_wide.hpp"       // (ahead of the kernel template: it declares the critic body's specialisation)
#include "ppo_update_fwd_bwd.hpp"

namespace ppoaf {

template <int HA, int HC>
static int fwd_bwd_launch_wide_pair(const FwdBwdLaunch& L) {
    static_assert(HC / 16 == kWideHT, "the wide body is the 512-wide critic's");
    return launch_fwd_bwd_as<HA / 16, HC / 16, true>(L.u, L.lds, L.s, L.e0, L.e1);
}

int fwd_bwd_launch_wide(const FwdBwdLaunch& L) {
    const int ha = L.u.net[0].H, hc = L.u.net[1].H;
    PPOAF_REQUIRE(L.u.split, "ppo_update_fwd_bwd: the wide pair (actor %d, critic %d) has no slab form: args->split_workspace is not set",
                  ha, hc);
#define PPOAF_WIDTH_PAIR_CALL_(A, C) fwd_bwd_launch_wide_pair<A, C>(L)
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_WIDE, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("ppo_update_fwd_bwd: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

}  // namespace ppoaf
