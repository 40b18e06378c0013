// K21: one env step of an LSTM actor / critic pair for every row of a rank in ONE launch:
//   STEP         actor forward -> distribution -> sample (Philox) -> log-prob          policies/ppo_policy.py:729-794
//                critic forward -> value -> denormalise                                ppo.py:1052-1075, utils/misc.py:113-128
//                + row t of the rollout buffer: observation copies, actions, log-probs, values and the four hidden rows
//                                                                                      policies/ppo_policy.py:593-651
//   CRITIC_NEXT  V(next critic observation) -> boot_value[t]; the critic's (h, c) are replaced only when the device
//                byte *commit is set (an episode was cut at this step)                 ppo.py:1863-1881
//                + the stored hidden rows of the envs that terminated at this step are zeroed
//                                                                                      policies/ppo_policy.py:593-627
//   INFER        actor forward -> the ENVIRONMENT action (K19's heads)                 policies/ppo_policy.py:796-889
//   MASK         the zeroing alone, for the steps without a CRITIC_NEXT launch
//
// STEP runs 2 * ceil(E/16) workgroups, XCD-grouped like K6 (blocks 0-3 mod 8 actor, 4-7 critic); the other modes one
// workgroup per 16 rows.  A workgroup has H / 16 waves (H = the LSTM width of BOTH networks).  The recurrence, LayerNorm
// and feed-forward head are K18's forward at S = 1 (lstm_device.hpp: lstm_rows_forward), the heads run one lane per row
// on K6's / K19's functions (action_heads.hpp).  The networks' (h, c) are stepped IN PLACE: a workgroup reads only its
// own 16 rows, all before its first barrier, and writes them after the recurrent step.
//
// Block form (ppoaf_lstm_policy_step_blocks, STEP and CRITIC_NEXT): the observations are read where the env left them,
// through a table of row blocks in the kernel arguments, and STEP also writes the env's action blocks -- a member of a
// multi-policy run then needs no gather and no index_put (PPO.rollout, DESIGN.md "LSTM members").
#include <cstddef>

#include "action_heads.hpp"
#include "lstm_device.hpp"

namespace ppoaf {

struct LstmStepDev {
    LstmArgs net[2];                               // actor, critic
    long E;
    int n_wg, mode, head_kind, infer_mode;
    float min_std;
    const float* log_std;
    const float* act_lo; const float* act_hi;
    const void* forced_raw_action;
    unsigned long long seed, offset;
    int normalize_values; const float* vn_mean; const float* vn_var;
    void* raw_action_out; void* action_out; float* logp_out;
    float* value_out;                              // values[t] (STEP) or boot_value[t] (CRITIC_NEXT)
    float* obs_out; float* critic_obs_out;
    const unsigned char* terminated;
    float* stored[4];                              // the step's hidden rows, for the zeroing
};

// The block form (ppoaf_lstm_policy_step_blocks): row r of the launch is row r % rows_per_block of block
// r / rows_per_block of `obs` / `critic_obs`, its env action (STEP) also goes to that row of `env_action`, and
// `terminated` (CRITIC_NEXT) holds one byte per row of a block.  The pointers travel in the kernel arguments.
struct LstmStepBlocks {
    const float* obs[PPOAF_ROW_BLOCKS_MAX];
    const float* critic_obs[PPOAF_ROW_BLOCKS_MAX];
    void* env_action[PPOAF_ROW_BLOCKS_MAX];
    unsigned rows_per_block;
    int action_elems;                              // float32 elements of a Gaussian row's env action; int64: 1
};

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_policy_step_kernel(const LstmStepDev u) {
    constexpr int NT = H / 16 * 64;
    const int tid = threadIdx.x;
    int which, g;
    if (u.mode == PPOAF_LSTM_STEP) {
        const int b = blockIdx.x;
        which = (b >> 2) & 1;
        g = ((b >> 3) << 2) | (b & 3);
    } else {
        which = u.mode == PPOAF_LSTM_INFER ? 0 : 1;
        g = blockIdx.x;
    }
    if (g >= u.n_wg) return;
    const long e0 = (long)g * kLRows;

    if (u.mode != PPOAF_LSTM_MASK) {
        const LstmArgs& a = u.net[which];
        float* oc = which == 0 ? u.obs_out : u.critic_obs_out;
        if (oc) {
            const long lo = e0 * a.I, hi = (e0 + kLRows < u.E ? e0 + kLRows : u.E) * a.I;
            for (long i = lo + tid; i < hi; i += NT) oc[i] = a.x[i];
        }
        const float* sOut = lstm_rows_forward<H, true>(a, g);

        // heads: one lane per env row
        if (tid < kLRows && e0 + tid < u.E) {
            const float* zr = sOut + tid * kLFS;
            const long e = e0 + tid;
            if (which == 1) {
                float v = zr[0];
                if (u.normalize_values) v = u.vn_mean[0] + v * sqrtf(u.vn_var[0] + 1e-8f);   // misc.py:124-128
                u.value_out[e] = v;
            } else if (u.mode == PPOAF_LSTM_INFER) {
                const bool greedy = u.infer_mode == PPOAF_INFER_DETERMINISTIC;
                if (u.head_kind == PPOAF_HEAD_CATEGORICAL)
                    cat_infer_row(zr, a.O, greedy, e, u.seed, u.offset, u.action_out);
                else
                    gauss_infer_row(zr, a.O, greedy, u.log_std, u.min_std, u.act_lo, u.act_hi, e, u.seed, u.offset,
                                    u.action_out);
            } else if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
                cat_step_row(zr, a.O, u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out, u.action_out, u.logp_out);
            } else {
                gauss_step_row(zr, a.O, u.log_std, u.min_std, u.act_lo, u.act_hi, u.forced_raw_action, e, u.seed, u.offset,
                               u.raw_action_out, u.action_out, u.logp_out);
            }
        }
    }

    // the rows the step stored for the envs that terminated at it: zero (the networks' own state is not reset)
    if (u.terminated && u.mode != PPOAF_LSTM_STEP && u.mode != PPOAF_LSTM_INFER) {
        for (int i = tid; i < kLRows * H; i += NT) {
            const int r = i / H;
            const long n = e0 + r;
            if (n < u.E && u.terminated[n]) {
                const long at = n * H + (i - r * H);
#pragma unroll
                for (int q = 0; q < 4; ++q) u.stored[q][at] = 0.f;
            }
        }
    }
}

// The block form of lstm_policy_step_kernel, STEP and CRITIC_NEXT only (the entry point refuses the other modes).  The
// tensor form keeps its own text and with it its code; both instantiate lstm_rows_forward and call the same head
// functions with the same row number, so for equal inputs they store equal bits.
template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_policy_step_blocks_kernel(const LstmStepDev u, const LstmStepBlocks tb) {
    constexpr int NT = H / 16 * 64;
    const int tid = threadIdx.x;
    int which = 1, g = blockIdx.x;
    if (u.mode == PPOAF_LSTM_STEP) {
        const int b = blockIdx.x;
        which = (b >> 2) & 1;
        g = ((b >> 3) << 2) | (b & 3);
    }
    if (g >= u.n_wg) return;
    const long e0 = (long)g * kLRows;
    const LstmArgs& a = u.net[which];
    const LstmXBlocks xr{which == 0 ? tb.obs : tb.critic_obs, tb.rows_per_block};
    float* oc = which == 0 ? u.obs_out : u.critic_obs_out;
    if (oc) {
        const int I = a.I;
        for (int i = tid; i < kLRows * I; i += NT) {
            const int r = i / I, k = i - r * I;
            if (e0 + r < u.E) oc[(e0 + r) * I + k] = xr.row(e0 + r, I)[k];
        }
    }
    const float* sOut = lstm_rows_forward<H, true, LstmXBlocks>(a, g, xr);

    // heads: one lane per env row
    if (tid < kLRows && e0 + tid < u.E) {
        const float* zr = sOut + tid * kLFS;
        const long e = e0 + tid;
        if (which == 1) {
            float v = zr[0];
            if (u.normalize_values) v = u.vn_mean[0] + v * sqrtf(u.vn_var[0] + 1e-8f);   // misc.py:124-128
            u.value_out[e] = v;
        } else {
            // the row's env action, as this lane stores it in the buffer row, also into the env's action tensor
            const unsigned b = (unsigned)e / tb.rows_per_block;
            const long r = (long)((unsigned)e - b * tb.rows_per_block);
            if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
                cat_step_row(zr, a.O, u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out, u.action_out, u.logp_out);
                reinterpret_cast<int64_t*>(tb.env_action[b])[r] = reinterpret_cast<const int64_t*>(u.action_out)[e];
            } else {
                gauss_step_row(zr, a.O, u.log_std, u.min_std, u.act_lo, u.act_hi, u.forced_raw_action, e, u.seed, u.offset,
                               u.raw_action_out, u.action_out, u.logp_out);
                const int n = tb.action_elems;
                const float* src = reinterpret_cast<const float*>(u.action_out) + e * n;
                float* dst = reinterpret_cast<float*>(tb.env_action[b]) + r * n;
                for (int k = 0; k < n; ++k) dst[k] = src[k];
            }
        }
    }

    // CRITIC_NEXT: the rows the step stored for the envs that terminated at it are zeroed; the env's byte serves each of
    // its agents' rows
    if (u.terminated && u.mode == PPOAF_LSTM_CRITIC_NEXT) {
        for (int i = tid; i < kLRows * H; i += NT) {
            const int r = i / H;
            const long n = e0 + r;
            if (n < u.E && u.terminated[(unsigned)n % tb.rows_per_block]) {
                const long at = n * H + (i - r * H);
#pragma unroll
                for (int q = 0; q < 4; ++q) u.stored[q][at] = 0.f;
            }
        }
    }
}

template <int H>
static int launch_lstm_step(const LstmStepDev& u, hipStream_t s) {
    const unsigned grid = u.mode == PPOAF_LSTM_STEP ? 8u * (unsigned)((u.n_wg + 3) / 4) : (unsigned)u.n_wg;
    hipLaunchKernelGGL(lstm_policy_step_kernel<H>, dim3(grid), dim3(H / 16 * 64), 0, s, u);
    return check_launch("lstm_policy_step");
}

template <int H>
static int launch_lstm_step_blocks(const LstmStepDev& u, const LstmStepBlocks& tb, hipStream_t s) {
    const unsigned grid = u.mode == PPOAF_LSTM_STEP ? 8u * (unsigned)((u.n_wg + 3) / 4) : (unsigned)u.n_wg;
    hipLaunchKernelGGL(lstm_policy_step_blocks_kernel<H>, dim3(grid), dim3(H / 16 * 64), 0, s, u, tb);
    return check_launch("lstm_policy_step_blocks");
}

// with_obs: obs / critic_obs are read from `a` (the block form reads them through its table)
static int check_step_args(const ppoaf_lstm_policy_step_args_t* a, const bool with_obs = true) {
    PPOAF_REQUIRE(a, "lstm_policy_step: null args");
    PPOAF_REQUIRE(a->mode >= PPOAF_LSTM_STEP && a->mode <= PPOAF_LSTM_MASK,
                  "lstm_policy_step: mode=%d (0 step, 1 critic next, 2 infer, 3 mask)", a->mode);
    if (int rc = check_lstm_desc(&a->actor, false, "lstm_policy_step: actor")) return rc;
    if (int rc = check_lstm_desc(&a->critic, false, "lstm_policy_step: critic")) return rc;
    PPOAF_REQUIRE(a->actor.hidden == a->critic.hidden,
                  "lstm_policy_step: LSTM hidden sizes differ (actor %d, critic %d): one launch has one block size",
                  a->actor.hidden, a->critic.hidden);
    PPOAF_REQUIRE(a->actor.steps == 1 && a->critic.steps == 1, "lstm_policy_step: steps must be 1");
    PPOAF_REQUIRE(a->critic.out_dim == 1, "lstm_policy_step: critic out_dim must be 1");
    PPOAF_REQUIRE(a->E >= 0, "lstm_policy_step: negative E");
    PPOAF_REQUIRE(a->E <= (1L << 27), "lstm_policy_step: E too large");
    PPOAF_REQUIRE(a->head_kind == PPOAF_HEAD_CATEGORICAL || a->head_kind == PPOAF_HEAD_GAUSSIAN,
                  "lstm_policy_step: head_kind=%d (0 categorical, 1 Gaussian)", a->head_kind);
    PPOAF_REQUIRE(a->head_kind != PPOAF_HEAD_GAUSSIAN || a->log_std, "lstm_policy_step: the Gaussian head needs log_std");
    PPOAF_REQUIRE((a->act_lo == nullptr) == (a->act_hi == nullptr), "lstm_policy_step: give both action bounds or neither");
    const bool rows = a->actor_hidden_out && a->actor_cell_out && a->critic_hidden_out && a->critic_cell_out;
    if (a->mode == PPOAF_LSTM_STEP) {
        PPOAF_REQUIRE((!with_obs || (a->obs && a->critic_obs)) && a->actor_h && a->actor_c && a->critic_h && a->critic_c,
                      "lstm_policy_step: STEP: null observation / state pointer");
        PPOAF_REQUIRE(a->raw_action_out && a->action_out && a->logp_out && a->value_out && rows,
                      "lstm_policy_step: STEP needs the row-t outputs (actions, log-probs, values, four hidden rows)");
    } else if (a->mode == PPOAF_LSTM_CRITIC_NEXT) {
        PPOAF_REQUIRE((!with_obs || a->critic_obs) && a->critic_h && a->critic_c && a->boot_value_out && a->commit,
                      "lstm_policy_step: CRITIC_NEXT: null critic_obs / critic state / boot_value_out / commit");
        PPOAF_REQUIRE(!a->terminated || rows, "lstm_policy_step: terminated given without the four hidden rows");
    } else if (a->mode == PPOAF_LSTM_INFER) {
        PPOAF_REQUIRE(a->obs && a->actor_h && a->actor_c && a->action_out,
                      "lstm_policy_step: INFER: null obs / actor state / action_out");
        PPOAF_REQUIRE(a->infer_mode == PPOAF_INFER_SAMPLE || a->infer_mode == PPOAF_INFER_DETERMINISTIC,
                      "lstm_policy_step: infer_mode=%d (0 sample, 1 deterministic)", a->infer_mode);
    } else {
        PPOAF_REQUIRE(a->terminated && rows, "lstm_policy_step: MASK needs terminated and the four hidden rows");
    }
    if (a->mode == PPOAF_LSTM_STEP || a->mode == PPOAF_LSTM_CRITIC_NEXT)
        PPOAF_REQUIRE(!a->normalize_values || (a->vn_mean && a->vn_var), "lstm_policy_step: normaliser state missing");
    return PPOAF_OK;
}

static int check_step_blocks(const ppoaf_lstm_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t) {
    PPOAF_REQUIRE(a && t, "lstm_policy_step_blocks: null args");
    PPOAF_REQUIRE(a->mode == PPOAF_LSTM_STEP || a->mode == PPOAF_LSTM_CRITIC_NEXT,
                  "lstm_policy_step_blocks: mode=%d (0 step, 1 critic next; INFER and MASK have no block form)", a->mode);
    PPOAF_REQUIRE(t->n_blocks >= 1 && t->n_blocks <= PPOAF_ROW_BLOCKS_MAX, "lstm_policy_step_blocks: n_blocks=%d not in [1, %d]",
                  t->n_blocks, PPOAF_ROW_BLOCKS_MAX);
    PPOAF_REQUIRE(t->rows_per_block >= 0, "lstm_policy_step_blocks: rows_per_block=%ld must be >= 0", (long)t->rows_per_block);
    PPOAF_REQUIRE(a->E == t->rows_per_block * t->n_blocks,
                  "lstm_policy_step_blocks: E=%ld is not n_blocks=%d x rows_per_block=%ld", (long)a->E, t->n_blocks,
                  (long)t->rows_per_block);
    // scalar loads and stores: the element's own alignment is all that is asked for
    const uintptr_t act_mask = a->head_kind == PPOAF_HEAD_GAUSSIAN ? 3 : 7;
    for (int b = 0; b < t->n_blocks; ++b) {
        PPOAF_REQUIRE(t->critic_obs[b] && ((uintptr_t)t->critic_obs[b] & 3) == 0,
                      "lstm_policy_step_blocks: block %d: the critic_obs base is null or not aligned to 4 bytes", b);
        if (a->mode == PPOAF_LSTM_STEP)
            PPOAF_REQUIRE(t->obs[b] && t->env_action[b] && ((uintptr_t)t->obs[b] & 3) == 0 &&
                              ((uintptr_t)t->env_action[b] & act_mask) == 0,
                          "lstm_policy_step_blocks: block %d: the obs / env_action base is null or not aligned to its element "
                          "(float32 4 bytes, int64 8)", b);
    }
    return check_step_args(a, false);
}

}  // namespace ppoaf

using namespace ppoaf;

// the layout the ctypes structure of _lib.py restates (tests/test_lstm_step_abi.py reads this list)
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, actor, 0);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic, 72);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, obs, 144);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_obs, 152);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, E, 160);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, actor_h, 168);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, actor_c, 176);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_h, 184);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_c, 192);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, head_kind, 200);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, min_std, 204);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, log_std, 208);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, act_lo, 216);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, act_hi, 224);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, forced_raw_action, 232);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, seed, 240);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, offset, 248);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, normalize_values, 256);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, mode, 260);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, vn_mean, 264);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, vn_var, 272);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, raw_action_out, 280);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, action_out, 288);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, logp_out, 296);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, value_out, 304);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, obs_copy_out, 312);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_obs_copy_out, 320);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, actor_hidden_out, 328);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, actor_cell_out, 336);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_hidden_out, 344);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, critic_cell_out, 352);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, infer_mode, 360);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, _pad, 364);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, commit, 368);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, terminated, 376);
PPOAF_LAYOUT(ppoaf_lstm_policy_step_args_t, boot_value_out, 384);
static_assert(sizeof(ppoaf_lstm_policy_step_args_t) == 392, "ppoaf_lstm_policy_step_args_t");

extern "C" int ppoaf_lstm_policy_step_check(const ppoaf_lstm_policy_step_args_t* a) { return check_step_args(a); }

// the device view of checked arguments
static LstmStepDev step_dev_of(const ppoaf_lstm_policy_step_args_t* a) {
    LstmStepDev u{};
    // (the descriptors' own `rows` is not read: E rules)
    u.net[0] = lstm_args_of(&a->actor);
    u.net[1] = lstm_args_of(&a->critic);
    for (int w = 0; w < 2; ++w) { u.net[w].N = a->E; u.net[w].S = 1; u.net[w].stash = 0; u.net[w].ws = nullptr; }
    LstmArgs& ac = u.net[0];
    LstmArgs& cr = u.net[1];
    ac.x = a->obs; ac.h0 = ac.hn = a->actor_h; ac.c0 = ac.cn = a->actor_c;
    cr.x = a->critic_obs; cr.h0 = cr.hn = a->critic_h; cr.c0 = cr.cn = a->critic_c;
    u.value_out = a->value_out;
    if (a->mode == PPOAF_LSTM_STEP) {
        ac.hn_row = a->actor_hidden_out; ac.cn_row = a->actor_cell_out;
        cr.hn_row = a->critic_hidden_out; cr.cn_row = a->critic_cell_out;
        u.obs_out = a->obs_copy_out; u.critic_obs_out = a->critic_obs_copy_out;
    } else if (a->mode == PPOAF_LSTM_CRITIC_NEXT) {
        cr.commit = a->commit;
        u.value_out = a->boot_value_out;
    }
    u.E = a->E;
    u.n_wg = (int)((a->E + kLRows - 1) / kLRows);
    u.mode = a->mode; u.head_kind = a->head_kind; u.infer_mode = a->infer_mode; u.min_std = a->min_std;
    u.log_std = a->log_std; u.act_lo = a->act_lo; u.act_hi = a->act_hi;
    u.forced_raw_action = a->mode == PPOAF_LSTM_STEP ? a->forced_raw_action : nullptr;
    u.seed = a->seed; u.offset = a->offset;
    u.normalize_values = a->normalize_values; u.vn_mean = a->vn_mean; u.vn_var = a->vn_var;
    u.raw_action_out = a->raw_action_out; u.action_out = a->action_out; u.logp_out = a->logp_out;
    u.terminated = (a->mode == PPOAF_LSTM_CRITIC_NEXT || a->mode == PPOAF_LSTM_MASK) ? a->terminated : nullptr;
    u.stored[0] = a->actor_hidden_out; u.stored[1] = a->actor_cell_out;
    u.stored[2] = a->critic_hidden_out; u.stored[3] = a->critic_cell_out;
    return u;
}

extern "C" int ppoaf_lstm_policy_step(const ppoaf_lstm_policy_step_args_t* a, ppoaf_stream_t stream) {
    if (int rc = check_step_args(a)) return rc;
    if (a->E == 0) return PPOAF_OK;
    const LstmStepDev u = step_dev_of(a);
    hipStream_t s = (hipStream_t)stream;
    switch (a->actor.hidden) {
        case 32: return launch_lstm_step<32>(u, s);
        case 64: return launch_lstm_step<64>(u, s);
    }
    return launch_lstm_step<128>(u, s);
}

PPOAF_LAYOUT(ppoaf_lstm_step_blocks_t, n_blocks, 0);
PPOAF_LAYOUT(ppoaf_lstm_step_blocks_t, rows_per_block, 8);
PPOAF_LAYOUT(ppoaf_lstm_step_blocks_t, obs, 16);
PPOAF_LAYOUT(ppoaf_lstm_step_blocks_t, critic_obs, 144);
PPOAF_LAYOUT(ppoaf_lstm_step_blocks_t, env_action, 272);
static_assert(sizeof(ppoaf_lstm_step_blocks_t) == 400, "ppoaf_lstm_step_blocks_t");

extern "C" int ppoaf_lstm_policy_step_blocks_check(const ppoaf_lstm_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t) {
    return check_step_blocks(a, t);
}

extern "C" int ppoaf_lstm_policy_step_blocks(const ppoaf_lstm_policy_step_args_t* a, const ppoaf_lstm_step_blocks_t* t,
                                             ppoaf_stream_t stream) {
    if (int rc = check_step_blocks(a, t)) return rc;
    if (a->E == 0) return PPOAF_OK;                 // no row: nothing is read, nothing launched
    LstmStepDev u = step_dev_of(a);
    u.net[0].x = u.net[1].x = nullptr;
    LstmStepBlocks tb;
    for (int b = 0; b < PPOAF_ROW_BLOCKS_MAX; ++b) {
        const bool in = b < t->n_blocks;
        tb.obs[b] = in && a->mode == PPOAF_LSTM_STEP ? t->obs[b] : nullptr;
        tb.critic_obs[b] = in ? t->critic_obs[b] : nullptr;
        tb.env_action[b] = in && a->mode == PPOAF_LSTM_STEP ? t->env_action[b] : nullptr;
    }
    tb.rows_per_block = (unsigned)t->rows_per_block;
    tb.action_elems = a->head_kind == PPOAF_HEAD_GAUSSIAN ? a->actor.out_dim : 1;
    hipStream_t s = (hipStream_t)stream;
    switch (a->actor.hidden) {
        case 32: return launch_lstm_step_blocks<32>(u, tb, s);
        case 64: return launch_lstm_step_blocks<64>(u, tb, s);
    }
    return launch_lstm_step_blocks<128>(u, tb, s);
}
