// K19: one evaluation step for every env row in ONE launch, actor only:
//   actor MLP forward -> head -> the ENVIRONMENT action                 policies/ppo_policy.py:796-889
//   deterministic: the distribution's refine_prediction                 networks/distributions.py:177-196 (Bernoulli),
//                  :262-263 (categorical), :404-436 (multi-categorical), :580-581,611-631 (Gaussian)
// and the score bookkeeping of testing.py:59-112 for E environments (ppoaf_eval_scores_step).
//
// grid = ceil(E/16) workgroups of 512 threads, 16 rows each.  The forward is mlp_rows_forward (mlp_device.hpp), the code
// K6 (policy_step.hip) instantiates for its actor half, and sampling goes through K6's own pieces (action_heads.hpp) with
// K6's Philox counters: for equal (obs, params, seed, offset) a sampled action is bitwise K6's action_out.  No critic,
// no log-prob, no buffer rows: half of K6's workgroups and all but one of its stores are not there.
// Actor outputs: <= 8; a 256-wide actor with 9 .. 24 outputs (Categorical, Gaussian) runs policy_wide_heads.hip's kernel.
#include "policy_rows.hpp"          // InferDev (shared with policy_wide_heads.hip)

namespace ppoaf {

template <int HT, bool XH>
__global__ __launch_bounds__(kThreadsU) void policy_infer_kernel(InferDev u) {
    const int tid = threadIdx.x;
    const NetDev& nd = u.net;
    const int out_dim = nd.out_dim;
    const long e0 = (long)blockIdx.x * kRows;
    const float* sOut = mlp_rows_forward<HT>(nd, u.params, u.obs, nullptr, u.E, e0, reinterpret_cast<float*>(policy_infer_smem));

    // heads: one lane per env row
    if (tid >= kRows || e0 + tid >= u.E) return;
    const float* zr = sOut + tid * kMaxOut;
    const long e = e0 + tid;
    const bool greedy = u.mode == PPOAF_INFER_DETERMINISTIC;
    if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
        cat_infer_row(zr, out_dim, greedy, e, u.seed, u.offset, u.action_out);
    } else if (XH) {
        float z[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = k < out_dim ? zr[k] : 0.f;
        if (u.head_kind == PPOAF_HEAD_MULTI_CATEGORICAL) {
            const int D = u.n_slices;
            const unsigned first = mcat_starts(D, u.slices);
            unsigned pick = 0u;
            if (greedy) {
                // per slice: the first class that holds the slice's maximum
                float t[8];
                slice_totals<true>(z, t, first);
                bool found = true;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k < out_dim) {
                        if ((first >> k) & 1u) found = false;
                        if (!found && z[k] == t[k]) { pick |= 1u << k; found = true; }
                    }
                }
            } else {
                float p[8], sm[8];
                mcat_probs(z, first, out_dim, p, sm);
                pick = mcat_sample(p, sm, first, out_dim, u.seed, u.offset, u.E, e);
            }
            int64_t* ac = reinterpret_cast<int64_t*>(u.action_out) + e * D;
            int j = -1, o = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < out_dim) {
                    if ((first >> k) & 1u) { ++j; o = k; }
                    if ((pick >> k) & 1u) ac[j] = k - o;
                }
            }
        } else {
            float* ac = reinterpret_cast<float*>(u.action_out) + e * out_dim;
            Philox4 r = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                if (d < out_dim) {
                    // greedy: p >= 0.5 <=> z >= 0 (sigmoid is monotone, sigmoid(0) = 0.5)
                    const bool on = greedy ? z[d] >= 0.f
                                           : bern_uniform(u.seed, u.offset + (unsigned long long)e, d, r) < sigmoid_u(z[d]);
                    ac[d] = on ? 1.f : 0.f;
                }
            }
        }
    } else {
        gauss_infer_row(zr, out_dim, greedy, u.params + nd.offset + nd.log_std_off, u.min_std, u.act_lo, u.act_hi, e,
                        u.seed, u.offset, u.action_out);
    }
}

template <int HT, bool XH>
static int launch_infer(const InferDev& u, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(policy_infer_kernel<HT, XH>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PPOAF_E_LAUNCH; }
        attr_set = true;
    }
    const unsigned grid = (unsigned)((u.E + kRows - 1) / kRows);
    hipLaunchKernelGGL((policy_infer_kernel<HT, XH>), dim3(grid), dim3(kThreadsU), lds, s, u);
    return check_launch("policy_infer");
}

template <bool XH>
static int launch_infer_width(const InferDev& u, size_t lds, hipStream_t s) {
    switch (u.net.H) {
        case 32: return launch_infer<2, XH>(u, lds, s);
        case 64: return launch_infer<4, XH>(u, lds, s);
        case 128: return launch_infer<8, XH>(u, lds, s);
        case 256: return launch_infer<16, XH>(u, lds, s);
    }
    set_error("policy_infer: hidden width %d not instantiated (32, 64, 128, 256)", u.net.H);
    return PPOAF_E_INVALID;
}

// ---- score bookkeeping, one thread per env row
struct ScoresDev {
    const float* score; const uint8_t* done; const int32_t* quota; long E;
    double* run_score; int64_t* run_len;
    int64_t* count; double* sum; double* min; double* max; int64_t* steps;
    int32_t* remaining;
};

__global__ __launch_bounds__(256) void eval_scores_kernel(ScoresDev u) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= u.E) return;
    const int64_t c = u.count[e];
    if (c >= (int64_t)u.quota[e]) return;                 // this row has delivered what it owes
    double rs = u.run_score[e] + (double)u.score[e];
    int64_t rl = u.run_len[e] + 1;
    if (u.done[e]) {
        u.count[e] = c + 1;
        u.sum[e] += rs;
        u.min[e] = fmin(u.min[e], rs);
        u.max[e] = fmax(u.max[e], rs);
        u.steps[e] += rl;
        rs = 0.0;
        rl = 0;
        atomicSub(u.remaining, 1);
    }
    u.run_score[e] = rs;
    u.run_len[e] = rl;
}

// ---- the books of a multi-agent evaluation, one thread per (book, env row): the chain of eval_scores_kernel launches
// testing.py made per agent and per policy, call for call in a register
struct BooksDev {
    const float* score; const uint8_t* done; const int32_t* quota; long E;
    int A, n_books; unsigned mask[32];
    double* run_score; int64_t* run_len;
    int64_t* count; double* sum; double* min; double* max; int64_t* steps;
    int32_t* remaining;
};

__global__ __launch_bounds__(256) void eval_scores_books_kernel(BooksDev u) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= u.E * u.n_books) return;
    const int b = (int)(i / u.E);
    const long e = i - (long)b * u.E;
    const int64_t c = u.count[i];
    if (c >= (int64_t)u.quota[e]) return;                 // (the count moves only where the episode closes: one test serves the chain)
    const unsigned mask = u.mask[b];
    double rs = u.run_score[i];
    int64_t rl = u.run_len[i];
    for (int a = 0; a < u.A; ++a) {
        if (!((mask >> a) & 1u)) continue;
        rs += (double)u.score[(long)a * u.E + e];
        rl += 1;
    }
    if (u.done[e]) {                                      // with the last agent of the mask
        u.count[i] = c + 1;
        u.sum[i] += rs;
        u.min[i] = fmin(u.min[i], rs);
        u.max[i] = fmax(u.max[i], rs);
        u.steps[i] += rl;
        rs = 0.0;
        rl = 0;
        atomicSub(u.remaining + b, 1);
    }
    u.run_score[i] = rs;
    u.run_len[i] = rl;
}

}  // namespace ppoaf

using namespace ppoaf;

// the layouts the ctypes structures of _lib.py restate (tests/test_eval_abi.py reads this list)
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, actor, 0);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, params, 48);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, obs, 56);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, E, 64);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, head_kind, 72);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, mode, 76);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, min_std, 80);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, n_action_slices, 84);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, action_slices, 88);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, act_lo, 120);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, act_hi, 128);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, seed, 136);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, offset, 144);
PPOAF_LAYOUT(ppoaf_policy_infer_args_t, action_out, 152);
static_assert(sizeof(ppoaf_policy_infer_args_t) == 160, "ppoaf_policy_infer_args_t");
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, score, 0);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, done, 8);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, quota, 16);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, E, 24);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, run_score, 32);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, run_len, 40);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, count, 48);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, sum, 56);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, min, 64);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, max, 72);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, steps, 80);
PPOAF_LAYOUT(ppoaf_eval_scores_args_t, remaining, 88);
static_assert(sizeof(ppoaf_eval_scores_args_t) == 96, "ppoaf_eval_scores_args_t");
PPOAF_LAYOUT(ppoaf_eval_books_args_t, score, 0);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, done, 8);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, quota, 16);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, E, 24);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, num_agents, 32);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, n_books, 36);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, book_mask, 40);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, run_score, 168);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, run_len, 176);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, count, 184);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, sum, 192);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, min, 200);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, max, 208);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, steps, 216);
PPOAF_LAYOUT(ppoaf_eval_books_args_t, remaining, 224);
static_assert(sizeof(ppoaf_eval_books_args_t) == 232, "ppoaf_eval_books_args_t");

extern "C" int ppoaf_policy_infer(const ppoaf_policy_infer_args_t* a, ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a, "policy_infer: null args");
    InferDev u;
    int rc = fill_net(a->actor, u.net, "actor");
    if (rc) return rc;
    PPOAF_REQUIRE(a->E >= 0, "policy_infer: negative E");
    PPOAF_REQUIRE(a->E <= (1L << 27), "policy_infer: E too large");
    PPOAF_REQUIRE(a->mode == PPOAF_INFER_SAMPLE || a->mode == PPOAF_INFER_DETERMINISTIC,
                  "policy_infer: mode=%d (0 sample, 1 deterministic)", a->mode);
    rc = check_action_head("policy_infer", a->head_kind, a->actor,
                           a->head_kind == PPOAF_HEAD_MULTI_CATEGORICAL ? a->n_action_slices : 0, a->action_slices);
    if (rc) return rc;
    rc = check_wide_head("policy_infer", a->actor, a->head_kind, 0);
    if (rc) return rc;
    PPOAF_REQUIRE(a->params && a->obs && a->action_out, "policy_infer: null pointer");
    PPOAF_REQUIRE((a->act_lo == nullptr) == (a->act_hi == nullptr), "policy_infer: give both action bounds or neither");
    if (a->E == 0) return PPOAF_OK;
    u.params = a->params; u.obs = a->obs; u.E = a->E;
    u.head_kind = a->head_kind; u.mode = a->mode; u.min_std = a->min_std;
    u.act_lo = a->act_lo; u.act_hi = a->act_hi;
    u.seed = a->seed; u.offset = a->offset; u.action_out = a->action_out;
    u.n_slices = a->head_kind == PPOAF_HEAD_MULTI_CATEGORICAL ? a->n_action_slices : 0;
    for (int j = 0; j < 8; ++j) u.slices[j] = j < u.n_slices ? a->action_slices[j] : 0;
    const size_t lds = (mlp_rows_forward_lds_floats(u.net) * 4 + 15) / 16 * 16;
    PPOAF_REQUIRE(lds <= 160 * 1024, "policy_infer: needs %zu B of LDS", lds);
    hipStream_t s = (hipStream_t)stream;
    if (u.net.out_dim > 8) return launch_infer_wide_heads(u, lds, s);         // (a 256-wide actor, Categorical or Gaussian: checked above)
    return u.head_kind >= PPOAF_HEAD_MULTI_CATEGORICAL ? launch_infer_width<true>(u, lds, s) : launch_infer_width<false>(u, lds, s);
}

extern "C" int ppoaf_eval_scores_step(const ppoaf_eval_scores_args_t* a, ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a, "eval_scores_step: null args");
    PPOAF_REQUIRE(a->E >= 0 && a->E <= (1L << 27), "eval_scores_step: E=%ld out of range", (long)a->E);
    PPOAF_REQUIRE(a->score && a->done && a->quota && a->run_score && a->run_len && a->count && a->sum && a->min &&
                      a->max && a->steps && a->remaining,
                  "eval_scores_step: null pointer");
    if (a->E == 0) return PPOAF_OK;
    ScoresDev u{a->score, a->done, a->quota, (long)a->E, a->run_score, a->run_len, a->count, a->sum, a->min, a->max,
                a->steps, a->remaining};
    hipLaunchKernelGGL(eval_scores_kernel, dim3((unsigned)((a->E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u);
    return check_launch("eval_scores_step");
}

extern "C" int ppoaf_eval_scores_step_books(const ppoaf_eval_books_args_t* a, ppoaf_stream_t stream) {
    PPOAF_REQUIRE(a, "eval_scores_step_books: null args");
    PPOAF_REQUIRE(a->E >= 0 && a->E <= (1L << 27), "eval_scores_step_books: E=%ld out of range", (long)a->E);
    PPOAF_REQUIRE(a->num_agents >= 1 && a->num_agents <= 16, "eval_scores_step_books: num_agents=%d out of [1,16]", a->num_agents);
    PPOAF_REQUIRE(a->n_books >= 1 && a->n_books <= 32, "eval_scores_step_books: n_books=%d out of [1,32]", a->n_books);
    for (int b = 0; b < a->n_books; ++b)
        PPOAF_REQUIRE(a->book_mask[b] > 0 && a->book_mask[b] < (1 << a->num_agents),
                      "eval_scores_step_books: book_mask[%d]=0x%x names no agent or one beyond %d", b, (unsigned)a->book_mask[b],
                      a->num_agents - 1);
    PPOAF_REQUIRE(a->score && a->done && a->quota && a->run_score && a->run_len && a->count && a->sum && a->min &&
                      a->max && a->steps && a->remaining,
                  "eval_scores_step_books: null pointer");
    if (a->E == 0) return PPOAF_OK;
    BooksDev u;
    u.score = a->score; u.done = a->done; u.quota = a->quota; u.E = (long)a->E;
    u.A = a->num_agents; u.n_books = a->n_books;
    for (int b = 0; b < 32; ++b) u.mask[b] = b < a->n_books ? (unsigned)a->book_mask[b] : 0u;
    u.run_score = a->run_score; u.run_len = a->run_len; u.count = a->count; u.sum = a->sum; u.min = a->min; u.max = a->max;
    u.steps = a->steps; u.remaining = a->remaining;
    const long n = u.E * u.n_books;
    hipLaunchKernelGGL(eval_scores_books_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u);
    return check_launch("eval_scores_step_books");
}
