// K23: the per-step bookkeeping of a rollout, one launch for all members (the policies of a multi-policy run, or a MAT
// team alone).  Replaces, per env step and per member, the torch statements of PPO.rollout that follow env.step:
// the gathers of the member's reward / natural-reward rows, `reward * ext_reward_weight`, `+ intrinsic`, the copies
// into buffer.rewards[t] and the natural-reward row, `end_kind[t]`, and -- once -- the shared ep_ts arithmetic
// (ppo.py:1795-1983 of the reference: terminated -> terminal end; ep_ts == max_ts_per_ep, truncated or the last step
// of the rollout -> bootstrapped end).
//
// The env's rewards arrive as a ROW-BLOCK TABLE per member: block b is the [E] reward row of the member's b-th agent
// (env order), wherever it lies -- a slice of the env's agent-major tensor or one tensor of a dict keyed by agent id.
// The pointers travel by value in the kernel arguments (no device-side table).
//
// One thread per env: it alone reads and writes ep_ts[e], so the update is in place and race-free, then walks the
// members and their blocks (at most 8 x 16 rows of work, three to five in the baselines).  Consecutive threads read
// consecutive floats of every block.  `reward * w` and `+ intrinsic` are two float32 roundings, as the two torch
// statements are (the library is built with -ffp-contract=off; __fmul_rn / __fadd_rn say so here as well).
#include <cstddef>
#include "common.hpp"

namespace ppoaf {

__global__ __launch_bounds__(256) void rollout_finish_rows_kernel(const ppoaf_rollout_finish_args_t a) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long E = a.E;
    if (e >= E) return;
    int kind = 0;
    if (a.write_ends) {
        const bool term = a.terminated[e] != 0;
        const bool trunc = a.truncated != nullptr && a.truncated[e] != 0;
        const int ts = a.ep_ts[e] + 1;
        const bool boot = !term && (ts >= a.max_ts_per_ep || trunc || a.last_step != 0);
        kind = term ? 1 : (boot ? 2 : 0);
        a.ep_ts[e] = (term || boot) ? 0 : ts;
    }
    const bool weigh = a.ext_reward_weight != 1.0f;
    for (int m = 0; m < a.n_members; ++m) {
        const ppoaf_finish_member_t& M = a.members[m];
        const int n = M.n_blocks;
        for (int s = 0; s < n; ++s) {
            // grouped: slot s of env e <- block slot_agent[s], row e * n + s; else block s, row s * E + e
            const int b = M.grouped ? M.slot_agent[s] : s;
            const long out = M.grouped ? e * n + s : (long)s * E + e;
            float r = M.reward[b][e];
            if (M.natural_out) M.natural_out[(long)b * E + e] = M.natural[b] ? M.natural[b][e] : r;
            if (weigh) r = __fmul_rn(r, a.ext_reward_weight);
            if (M.intrinsic) r = __fadd_rn(r, M.intrinsic[out]);
            M.reward_out[out] = r;
            if (a.write_ends && !M.grouped) M.end_kind_out[out] = (int8_t)kind;
        }
        if (a.write_ends && M.grouped) M.end_kind_out[e] = (int8_t)kind;
    }
}

}  // namespace ppoaf

using namespace ppoaf;

#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_finish_member_t, slot_agent, 8);
PPOAF_LAYOUT(ppoaf_finish_member_t, reward, 72);
PPOAF_LAYOUT(ppoaf_finish_member_t, natural, 200);
PPOAF_LAYOUT(ppoaf_finish_member_t, intrinsic, 328);
PPOAF_LAYOUT(ppoaf_finish_member_t, end_kind_out, 352);
static_assert(sizeof(ppoaf_finish_member_t) == 360, "ppoaf_finish_member_t");
PPOAF_LAYOUT(ppoaf_rollout_finish_args_t, ext_reward_weight, 16);
PPOAF_LAYOUT(ppoaf_rollout_finish_args_t, E, 24);
PPOAF_LAYOUT(ppoaf_rollout_finish_args_t, ep_ts, 48);
PPOAF_LAYOUT(ppoaf_rollout_finish_args_t, members, 56);
static_assert(sizeof(ppoaf_rollout_finish_args_t) == 2936, "ppoaf_rollout_finish_args_t (by value in the kernel arguments: < 4096)");
#undef PPOAF_LAYOUT

extern "C" int ppoaf_rollout_finish_rows(const ppoaf_rollout_finish_args_t* a, ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a, "rollout_finish_rows: null args");
    PPOAF_REQUIRE(a->E >= 0, "rollout_finish_rows: E=%ld must be >= 0", (long)a->E);
    PPOAF_REQUIRE(a->n_members >= 1 && a->n_members <= PPOAF_FINISH_MAX_MEMBERS, "rollout_finish_rows: n_members=%d not in [1, %d]",
                  a->n_members, PPOAF_FINISH_MAX_MEMBERS);
    for (int m = 0; m < a->n_members; ++m) {
        const ppoaf_finish_member_t& M = a->members[m];
        PPOAF_REQUIRE(M.n_blocks >= 1 && M.n_blocks <= PPOAF_ROW_BLOCKS_MAX, "rollout_finish_rows: member %d: n_blocks=%d not in [1, %d]",
                      m, M.n_blocks, PPOAF_ROW_BLOCKS_MAX);
        PPOAF_REQUIRE(M.grouped == 0 || M.grouped == 1, "rollout_finish_rows: member %d: grouped=%d (0 or 1)", m, M.grouped);
        unsigned seen = 0;
        for (int s = 0; s < M.n_blocks; ++s) {
            if (M.grouped) {
                const int b = M.slot_agent[s];
                PPOAF_REQUIRE(b >= 0 && b < M.n_blocks, "rollout_finish_rows: member %d: slot_agent[%d]=%d is outside the table of %d blocks",
                              m, s, b, M.n_blocks);
                PPOAF_REQUIRE(!(seen & (1u << b)), "rollout_finish_rows: member %d: slot_agent names block %d twice", m, b);
                seen |= 1u << b;
            }
            // rows of float32 read with scalar loads: the natural alignment is all the kernel needs (an env's reward rows
            // for E = 10 lie 40 bytes apart)
            PPOAF_REQUIRE(M.reward[s] != nullptr && ((uintptr_t)M.reward[s] & 3) == 0,
                          "rollout_finish_rows: member %d: reward block %d is null or not 4-byte aligned", m, s);
            PPOAF_REQUIRE(((uintptr_t)M.natural[s] & 3) == 0, "rollout_finish_rows: member %d: natural block %d is not 4-byte aligned", m, s);
        }
        PPOAF_REQUIRE(M.reward_out != nullptr && ((uintptr_t)M.reward_out & 3) == 0 && ((uintptr_t)M.natural_out & 3) == 0 &&
                      ((uintptr_t)M.intrinsic & 3) == 0, "rollout_finish_rows: member %d: reward_out null, or a row not 4-byte aligned", m);
        PPOAF_REQUIRE(!a->write_ends || M.end_kind_out != nullptr, "rollout_finish_rows: member %d: write_ends without end_kind_out", m);
    }
    if (a->write_ends) {
        PPOAF_REQUIRE(a->terminated && a->ep_ts && ((uintptr_t)a->ep_ts & 3) == 0, "rollout_finish_rows: write_ends needs terminated and ep_ts");
        PPOAF_REQUIRE(a->max_ts_per_ep >= 1, "rollout_finish_rows: max_ts_per_ep=%d", a->max_ts_per_ep);
    }
    if (a->E == 0) return PPOAF_OK;
    PPOAF_REQUIRE(a->E <= (1L << 31) - 256, "rollout_finish_rows: E=%ld too large", (long)a->E);
    const unsigned grid = (unsigned)((a->E + 255) / 256);
    hipLaunchKernelGGL(rollout_finish_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
    return check_launch("rollout_finish_rows");
}
