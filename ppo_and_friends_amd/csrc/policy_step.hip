// K6+K7: one rollout step for every env of a rank in ONE launch:
//   actor MLP forward -> distribution -> sample (Philox) -> log-prob      policies/ppo_policy.py:758-794
//   critic MLP forward -> value -> denormalise                            ppo.py:1052-1075, utils/misc.py:113-128
//   + the step's rows of the rollout buffer (observation copies, actions, log-probs, values)
//                                                                         policies/ppo_policy.py:638-651
// replacing, per step, two small-batch torch forwards with host round trips, torch.distributions on the
// CPU and E `EpisodeInfo.add_info` calls.
//
// grid = 2 * ceil(E/16) workgroups (XCD-grouped like the update kernel: blocks 0-3 mod 8 actor, 4-7
// critic), 512 threads: 16 env rows per workgroup, hidden layers on v_mfma_f32_16x16x4_f32 with the same
// tile code as the update's forward, so a row's log-prob here and in the first mini-batch agree bit for bit.
// Actor outputs: <= 8; the wide pair's actor (256 beside 512) with 9 .. 24 outputs under a Categorical or Gaussian head
// runs policy_wide_heads.hip's kernels (fill_step: check_wide_head).
#include "policy_rows.hpp"          // StepDev, StepBlocks and the 16-row body (shared with policy_wide_heads.hip)

namespace ppoaf {

template <int HTA, int HTC, bool XH>
__global__ __launch_bounds__(kThreadsS) void policy_step_kernel(StepDev u) {
    const int b = blockIdx.x;
    const int which = (b >> 2) & 1;
    const int g = ((b >> 3) << 2) | (b & 3);
    if (g >= u.n_wg) return;
    if (which == 0) policy_step_body<HTA, XH>(u, 0, g);
    else policy_step_body<HTC, XH>(u, 1, g);
}

template <int HTA, int HTC, bool XH>
__global__ __launch_bounds__(kThreadsS) void policy_step_blocks_kernel(StepDev u, StepBlocks tb) {
    const int b = blockIdx.x;
    const int which = (b >> 2) & 1;
    const int g = ((b >> 3) << 2) | (b & 3);
    if (g >= u.n_wg) return;
    if (which == 0) policy_step_body<HTA, XH, true>(u, 0, g, &tb);
    else policy_step_body<HTC, XH, true>(u, 1, g, &tb);
}

static size_t step_lds_bytes(const StepDev& u) {
    size_t worst = 0;
    for (int w = 0; w < 2; ++w) {
        const NetDev& n = u.net[w];
        const size_t f = mlp_rows_forward_lds_floats(n);
        if (f * 4 > worst) worst = f * 4;
    }
    return (worst + 15) / 16 * 16;
}

template <int HTA, int HTC, bool XH>
static int launch_step(const StepDev& u, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_step_kernel<HTA, HTC, XH>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = 8u * (unsigned)((u.n_wg + 3) / 4);
    hipLaunchKernelGGL((policy_step_kernel<HTA, HTC, XH>), dim3(grid), dim3(kThreadsS), lds, s, u);
    return check_launch("policy_step");
}

template <int HTA, int HTC, bool XH>
static int launch_step_blocks(const StepDev& u, const StepBlocks& tb, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_step_blocks_kernel<HTA, HTC, XH>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = 8u * (unsigned)((u.n_wg + 3) / 4);
    hipLaunchKernelGGL((policy_step_blocks_kernel<HTA, HTC, XH>), dim3(grid), dim3(kThreadsS), lds, s, u, tb);
    return check_launch("policy_step_blocks");
}

template <bool XH>
static int launch_widths_blocks(const StepDev& u, const StepBlocks& tb, size_t lds, hipStream_t s) {
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) launch_step_blocks<A / 16, C / 16, XH>(u, tb, lds, s)
    PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("policy_step_blocks: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

template <bool XH>
static int launch_widths(const StepDev& u, size_t lds, hipStream_t s) {
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) launch_step<A / 16, C / 16, XH>(u, lds, s)
    PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("policy_step: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

}  // namespace ppoaf

using namespace ppoaf;

// validates `a` and fills the device view; *empty: E == 0, nothing to launch.  with_obs: obs / critic_obs are read from `a`
static int fill_step(const ppoaf_policy_step_args_t* a, StepDev& u, bool with_obs, bool* empty, size_t* lds_out) {
    *empty = false;
    int rc = fill_net(a->actor, u.net[0], "actor");
    if (rc) return rc;
    rc = fill_net(a->critic, u.net[1], "critic");
    if (rc) return rc;
    rc = check_wide_head("policy_step", a->actor, a->head_kind, a->critic.hidden);       // (more than 8 actor outputs)
    if (rc) return rc;
    PPOAF_REQUIRE(a->E >= 0, "policy_step: negative E");
    if (a->E == 0) { *empty = true; return PPOAF_OK; }
    PPOAF_REQUIRE(a->E <= (1L << 27), "policy_step: E too large");
    PPOAF_REQUIRE(a->params && (!with_obs || (a->obs && a->critic_obs)) && a->raw_action_out && a->action_out &&
                      a->logp_out && a->value_out,
                  "policy_step: null pointer");
    PPOAF_REQUIRE(a->critic.out_dim == 1, "policy_step: critic out_dim must be 1");
    rc = check_action_head("policy_step", a->head_kind, a->actor,
                           a->head_kind == PPOAF_HEAD_MULTI_CATEGORICAL ? a->n_action_slices : 0, a->action_slices);
    if (rc) return rc;
    PPOAF_REQUIRE(!a->normalize_values || (a->vn_mean && a->vn_var), "policy_step: normaliser state missing");
    u.params = a->params; u.obs = a->obs; u.critic_obs = a->critic_obs; u.E = a->E;
    PPOAF_REQUIRE((a->act_lo == nullptr) == (a->act_hi == nullptr), "policy_step: give both action bounds or neither");
    u.head_kind = a->head_kind; u.min_std = a->min_std; u.act_lo = a->act_lo; u.act_hi = a->act_hi;
    u.forced_raw_action = a->forced_raw_action;
    u.seed = a->seed; u.offset = a->offset; u.normalize_values = a->normalize_values;
    u.vn_mean = a->vn_mean; u.vn_var = a->vn_var; u.raw_action_out = a->raw_action_out;
    u.action_out = a->action_out; u.logp_out = a->logp_out; u.value_out = a->value_out;
    u.obs_out = a->obs_copy_out; u.critic_obs_out = a->critic_obs_copy_out;
    u.n_wg = (int)((a->E + kRows - 1) / kRows);
    u.n_slices = a->head_kind == PPOAF_HEAD_MULTI_CATEGORICAL ? a->n_action_slices : 0;
    for (int j = 0; j < 8; ++j) u.slices[j] = j < u.n_slices ? a->action_slices[j] : 0;
    const size_t lds = step_lds_bytes(u);
    PPOAF_REQUIRE(lds <= 160 * 1024, "policy_step: needs %zu B of LDS", lds);
    *lds_out = lds;
    return PPOAF_OK;
}

extern "C" int ppoaf_policy_step(const ppoaf_policy_step_args_t* a, ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a, "policy_step: null args");
    StepDev u;
    bool empty;
    size_t lds = 0;
    const int rc = fill_step(a, u, true, &empty, &lds);
    if (rc || empty) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (u.net[0].out_dim > 8) return launch_step_wide_heads(u, lds, s);       // (fill_step has checked the pair and the head)
    return u.head_kind >= PPOAF_HEAD_MULTI_CATEGORICAL ? launch_widths<true>(u, lds, s) : launch_widths<false>(u, lds, s);
}

extern "C" int ppoaf_policy_step_blocks(const ppoaf_policy_step_args_t* a, const ppoaf_step_blocks_t* t,
                                        ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a && t, "policy_step_blocks: null args");
    PPOAF_REQUIRE(t->n_blocks >= 1 && t->n_blocks <= PPOAF_ROW_BLOCKS_MAX, "policy_step_blocks: n_blocks=%d not in [1, %d]",
                  t->n_blocks, PPOAF_ROW_BLOCKS_MAX);
    PPOAF_REQUIRE(t->rows_per_block >= 0, "policy_step_blocks: rows_per_block=%ld must be >= 0", (long)t->rows_per_block);
    PPOAF_REQUIRE(a->E == t->rows_per_block * t->n_blocks, "policy_step_blocks: E=%ld is not n_blocks=%d x rows_per_block=%ld",
                  (long)a->E, t->n_blocks, (long)t->rows_per_block);
    for (int b = 0; b < t->n_blocks; ++b)
        PPOAF_REQUIRE(t->obs[b] && t->critic_obs[b] && t->env_action[b] && ((uintptr_t)t->obs[b] & 15) == 0 &&
                          ((uintptr_t)t->critic_obs[b] & 15) == 0 && ((uintptr_t)t->env_action[b] & 15) == 0,
                      "policy_step_blocks: block %d: a base is null or not 16-byte aligned", b);
    if (a->E == 0) return PPOAF_OK;                 // no env: nothing is read, nothing launched
    StepDev u;
    bool empty;
    size_t lds = 0;
    const int rc = fill_step(a, u, false, &empty, &lds);
    if (rc || empty) return rc;
    StepBlocks tb;
    for (int b = 0; b < PPOAF_ROW_BLOCKS_MAX; ++b) {
        const bool in = b < t->n_blocks;
        tb.obs[b] = in ? t->obs[b] : nullptr;
        tb.critic_obs[b] = in ? t->critic_obs[b] : nullptr;
        tb.env_action[b] = in ? t->env_action[b] : nullptr;
    }
    tb.rows_per_block = t->rows_per_block;
    tb.action_is_float = u.head_kind == PPOAF_HEAD_GAUSSIAN || u.head_kind == PPOAF_HEAD_BERNOULLI;
    tb.action_elems = u.head_kind == PPOAF_HEAD_CATEGORICAL ? 1
                      : u.head_kind == PPOAF_HEAD_MULTI_CATEGORICAL ? u.n_slices : u.net[0].out_dim;
    u.obs = nullptr; u.critic_obs = nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (u.net[0].out_dim > 8) return launch_step_blocks_wide_heads(u, tb, lds, s);
    return u.head_kind >= PPOAF_HEAD_MULTI_CATEGORICAL ? launch_widths_blocks<true>(u, tb, lds, s)
                                                       : launch_widths_blocks<false>(u, tb, lds, s);
}

static_assert(offsetof(ppoaf_step_blocks_t, rows_per_block) == 8 && offsetof(ppoaf_step_blocks_t, obs) == 16 &&
                  offsetof(ppoaf_step_blocks_t, critic_obs) == 144 && offsetof(ppoaf_step_blocks_t, env_action) == 272 &&
                  sizeof(ppoaf_step_blocks_t) == 400, "ppoaf_step_blocks_t");
