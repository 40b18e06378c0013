// K12's fwd_bwd kernels for the narrow-actor width pairs (64, 256), (32, 256) and (32, 64): the row-tile body per network
// and, beside a 256-wide critic of depth 2 .. 4, the critic's tiles on workgroup pairs with one workgroup per actor tile.
// A translation unit of its own: ppo_update.hip, with the other six pairs, is the longest compile of the build already.
#include "ppo_update_fwd_bwd.hpp"

namespace ppoaf {

int fwd_bwd_launch_narrow(const FwdBwdLaunch& L) {
    const int ha = L.u.net[0].H, hc = L.u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) fwd_bwd_launch_pair<A, C>(L)
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_IN_NARROW, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("ppo_update_fwd_bwd: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

}  // namespace ppoaf
