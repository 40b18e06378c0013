// K22: one mini-batch of the PPO update of an LSTM actor / critic pair (ppo.py:2292-2469) as three launches that read
// the device cursor -- a whole epoch is enqueued without returning to the host and replayed from hipGraphs.
//   fwd_bwd  2 * ceil(B/16) workgroups (actor tiles, then critic tiles) of H / 16 waves.  Prologue: the tile's 16 items of
//            the shuffled permutation -> their observation windows (buffer rows row_map[item + s]; actor observations
//            zeroed strictly after a terminal position, episode_info.py:976-987) and the stored (h, c) of the LAST
//            position (ppo.py:2312-2319), staged into the workspace.  Then K18's forward body (lstm_device.hpp), the
//            final (h, c) back to the tables (ppo.py:2450-2466), K12's head + loss terms of the rows (ppo_update_dev.hpp:
//            ppo_head_loss; values scattered at the last position, ppo.py:2340) and K18's backward body.  A row's loss
//            gradient needs only the mini-batch's moment records, so nothing crosses workgroups.
//   wgrad    K18's weight-gradient tiles for both networks, stored (not added) into the policy's gradient bucket, a
//            squared-norm partial per workgroup; the last workgroup advances the Adam step counters.
//   adam     per-network clip norm + the shared Adam element step (wgrad_tile.hpp); the last workgroup folds the loss
//            partials into the totals in tile order, integrates the value normaliser's record and advances the cursor.
// No launch waits for another workgroup; none is a memset.
#include <cstddef>

#include "lstm_device.hpp"
#include "ppo_update_dev.hpp"
#include "running_stats_device.hpp"

namespace ppoaf {
namespace {

constexpr int kUpdMaxJobs = 2 * kLMaxJobs;
constexpr long kLdsCarve = 160 * 1024;             // LDS a gfx950 workgroup can be given

// per-network pieces of the workspace, float offsets: K18's stash, then what the prologue stages and the head leaves
struct UpdWs { long net, x, h0, c0, hn, cn, dout, dls, end; };

struct UpdLayout { UpdWs w[2]; long total; };

struct LstmUpdDev {
    LstmArgs net[2];                               // actor, critic (x / h0 / c0 / hn / cn / dout: the staged copies)
    int H;
    float* xs[2]; float* h0s[2]; float* c0s[2]; float* douts[2]; float* dls;
    const float* obs[2]; float* tab_h[2]; float* tab_c[2];
    const unsigned char* terminal;
    const int64_t* perm; const int32_t* row_map; long n_rows, n_items;
    const void* raw_actions; const float* adv; const float* old_lp; const float* rtg; float* values;
    int64_t* cursor; long B, batch_stride;
    int normalize_values, n_ranks;
    float* vn_mean; float* vn_var; double* vn_count; const double* vn_records; const double* adv_records;
    int normalize_adv, use_huber, head_kind;
    float surr_clip, entropy_weight, kl_loss_weight, huber_delta, min_std;
    const float* log_std;
    float* loss_partials; double* totals;
    int n_wg;
    int n_slices; int slices[8];                   // (ppo_head_loss's multi-categorical branch: never taken here)
    // optimiser
    float* params; float* grads; float* exp_avg; float* exp_avg_sq;
    long bucket_total, actor_size;
    int64_t* step_counts; const float* lr; double* norm_scratch;
    float beta1, beta2, adam_eps, grad_scale, max_norm;
};

struct UpdJobs {
    WJob j[kUpdMaxJobs];
    int n, first_critic_tile, n_tiles;
};

inline UpdLayout upd_layout(const ppoaf_lstm_update_args_t& a) {
    UpdLayout U{};
    long o = 0;
    for (int w = 0; w < 2; ++w) {
        ppoaf_lstm_desc_t d = w == 0 ? a.actor : a.critic;
        d.rows = a.B;
        const LstmLayout L = layout_of(d);
        const long B = a.B, S = d.steps, H = d.hidden;
        UpdWs& p = U.w[w];
        p.net = o; o += pad4(L.total);
        p.x = o; o += pad4(B * S * d.in_dim);
        p.h0 = o; o += B * H;
        p.c0 = o; o += B * H;
        p.hn = o; o += B * H;
        p.cn = o; o += B * H;
        p.dout = o; o += pad4(B * d.out_dim);
        p.dls = o; o += w == 0 ? B * 8 : 0;
        p.end = o;
    }
    U.total = o;
    return U;
}

// static LDS of a fwd_bwd workgroup: the forward body's x / h buffers, the backward body's dgates buffers (both in
// lstm_device.hpp) and the prologue / head arrays of lstm_update_fwd_bwd_kernel
inline long upd_lds_bytes(const int H) {
    const long HS = H + 4, GS = 4 * H + 4, XS = kLMaxIn + 4;
    const long fwd = 2 * kLRows * XS + 2 * kLRows * HS;
    const long b1 = 2 * kLRows * GS, b2 = 2 * kLRows * kLFS + kLRows * HS;
    const long own = kLRows * 16 /* sWin */ + kLRows /* sRow */ + 48 + 4 + kLRows * 8
                     + 2 * kLRows * kMaxOut;
    return 4 * (fwd + (b1 > b2 ? b1 : b2) + own);
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) void lstm_update_fwd_bwd_kernel(const LstmUpdDev u) {
    constexpr int NT = H / 16 * 64;
    __shared__ int sWin[kLRows * 16];              // buffer row of (tile row, step); -1: zeros
    __shared__ int sRow[kLRows];                   // buffer row of the item's last position; -1: dead row
    __shared__ float sRowF[48];
    __shared__ float sMisc[4];
    __shared__ float sActF[kLRows * 8];
    __shared__ float sOut[kLRows * kMaxOut];
    __shared__ float sDOut[kLRows * kMaxOut];
    const int tid = threadIdx.x;
    const int which = (int)blockIdx.x >= u.n_wg ? 1 : 0;
    const int g = (int)blockIdx.x - which * u.n_wg;
    const LstmArgs& a = u.net[which];
    const long B = u.B, r0 = (long)g * kLRows;
    const int S = a.S, I = a.I, O = a.O;
    const long mb = u.cursor[0];
    const long base = mb * u.batch_stride;

    // ---- prologue: the tile's items, their rows, the last position's scalars
    if (tid < kLRows) {
        const long n = r0 + tid;
        long item = -1;
        int row = -1;
        float av = 0.f, lpo = 0.f, rt = 0.f;
        if (n < B && base + n < u.n_items) {
            const long p = u.perm[base + n];
            if (p >= 0 && p + S <= u.n_rows) {
                const int r = u.row_map[p + S - 1];
                if (r >= 0 && r < u.n_rows) { item = p; row = r; }
            }
            if (row >= 0) {
                const long di = base + n;
                if (which == 0) {
                    av = u.adv[di]; lpo = u.old_lp[di];
                    if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
                        reinterpret_cast<int*>(sActF)[tid * 8] = (int)reinterpret_cast<const int64_t*>(u.raw_actions)[di];
                    } else {
                        for (int d = 0; d < O; ++d) sActF[tid * 8 + d] = reinterpret_cast<const float*>(u.raw_actions)[di * O + d];
                    }
                } else {
                    rt = u.rtg[di];
                }
            }
        }
        bool cut = false;                          // a terminal position lies before this step
        for (int s = 0; s < S; ++s) {
            int wr = -1;
            if (item >= 0 && !(which == 0 && cut)) {
                wr = u.row_map[item + s];
                if (wr < 0 || wr >= u.n_rows) wr = -1;
            }
            sWin[tid * 16 + s] = wr;
            if (item >= 0 && u.terminal && u.terminal[item + s]) cut = true;
        }
        sRow[tid] = row;
        sRowF[tid] = av; sRowF[16 + tid] = lpo; sRowF[32 + tid] = rt;
    }
    if (tid == 64) {
        float mean_f = 0.f, std_f = 1.f;
        if (which == 0 && u.normalize_adv) adv_mean_std(u.adv_records + mb * 3, mean_f, std_f);
        sMisc[0] = mean_f; sMisc[1] = std_f;
    }
    if (tid == 96) {
        float m = 0.f, v = 1.f;
        double cnt = 0.0;
        if (which == 1) minibatch_vn_state(u, mb, m, v, cnt);
        sMisc[2] = m; sMisc[3] = v;
    }
    __syncthreads();

    // ---- the windows and (h0, c0) into this tile's rows of the workspace (the weight-gradient launch reads them too)
    {
        const float* obs = u.obs[which];
        float* xs = u.xs[which];
        const int SI = S * I;
        for (int e = tid; e < kLRows * SI; e += NT) {
            const int r = e / SI, rem = e - r * SI, s = rem / I, k = rem - s * I;
            const long n = r0 + r;
            if (n < B) {
                const int wr = sWin[r * 16 + s];
                xs[(n * S + s) * I + k] = wr >= 0 ? obs[(long)wr * I + k] : 0.f;
            }
        }
        const float* th = u.tab_h[which];
        const float* tc = u.tab_c[which];
        for (int e = tid; e < kLRows * H; e += NT) {
            const int r = e / H, k = e - r * H;
            const long n = r0 + r;
            if (n < B) {
                const int row = sRow[r];
                u.h0s[which][n * H + k] = row >= 0 ? th[(long)row * H + k] : 0.f;
                u.c0s[which][n * H + k] = row >= 0 ? tc[(long)row * H + k] : 0.f;
            }
        }
    }
    __syncthreads();                               // (a workgroup reads back only what it wrote itself)

    const float* fo = lstm_rows_forward<H, true>(a, g);

    // ---- the final (h, c) replace the stored ones (rows of a mini-batch are distinct; this tile read its own above)
    for (int e = tid; e < kLRows * H; e += NT) {
        const int r = e / H, k = e - r * H;
        const long n = r0 + r;
        if (n < B && sRow[r] >= 0) {
            const long at = (long)sRow[r] * H + k;
            u.tab_h[which][at] = a.hn[n * H + k];
            u.tab_c[which][at] = a.cn[n * H + k];
        }
    }
    for (int e = tid; e < kLRows * kMaxOut; e += NT) {
        const int r = e / kMaxOut, k = e - r * kMaxOut;
        sOut[e] = k < O ? fo[r * kLFS + k] : 0.f;
    }
    __syncthreads();

    // ---- head + loss of the 16 rows by one wave (K12's), d loss / d out -> sDOut
    if (tid < 64) ppo_head_loss(u, which, g, O, u.log_std, sRow, sRowF, sMisc, sActF, sOut, sDOut, tid, B);
    __syncthreads();
    for (int e = tid; e < kLRows * O; e += NT) {
        const int r = e / O, o = e - r * O;
        const long n = r0 + r;
        if (n < B) u.douts[which][n * O + o] = sDOut[r * kMaxOut + o];
    }
    if (which == 0 && u.head_kind == PPOAF_HEAD_GAUSSIAN) {
        for (int e = tid; e < kLRows * 8; e += NT) {
            const int r = e >> 3, d = e & 7;
            const long n = r0 + r;
            if (n < B) u.dls[n * 8 + d] = (d < O && sRow[r] >= 0) ? sOut[r * kMaxOut + 8 + d] : 0.f;
        }
    }
    __syncthreads();

    lstm_rows_backward<H>(a, g);
}

__global__ __launch_bounds__(256) void lstm_update_wgrad_kernel(const UpdJobs J, const float grad_scale, int64_t* step_counts,
                                                                 double* norm_scratch) {
    __shared__ float part[4][64][4];
    __shared__ double red[17];
    const int b = blockIdx.x;
    if (b == J.n_tiles) {                          // bookkeeping: the step counters of the Adam step that follows
        if (threadIdx.x < 2) step_counts[threadIdx.x] += 1;
        return;
    }
    int ji = 0;
    while (ji + 1 < J.n && b >= J.j[ji + 1].tile_begin) ++ji;
    const WJob& jb = J.j[ji];
    const float v = lstm_wgrad_tile<false>(jb, b - jb.tile_begin, part) * grad_scale;
    double q = (double)v * v;
    if (jb.out2) q += q;
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
        const bool critic = b >= J.first_critic_tile;
        norm_scratch[2 + 2 * b] = critic ? 0.0 : q;
        norm_scratch[3 + 2 * b] = critic ? q : 0.0;
    }
}

// norm pass of the N > 1 all-reduce path: the squared norms of the (summed) scaled gradients, a pair of partials per workgroup
__global__ __launch_bounds__(256) void lstm_update_sqnorm_kernel(const LstmUpdDev u) {
    __shared__ double red[17];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    double q0 = 0.0, q1 = 0.0;
    if (idx < u.bucket_total) {
        const float s = u.grads[idx] * u.grad_scale;
        if (idx < u.actor_size) q0 = (double)s * s; else q1 = (double)s * s;
    }
    q0 = block_sum(q0, red);
    q1 = block_sum(q1, red);
    if (threadIdx.x == 0) { u.norm_scratch[2 + 2 * blockIdx.x] = q0; u.norm_scratch[3 + 2 * blockIdx.x] = q1; }
}

__device__ __forceinline__ void lstm_update_bookkeeping(const LstmUpdDev& u) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    float p0 = 0.f, p2 = 0.f, p3 = 0.f, p4 = 0.f, p7 = 0.f;
    for (int g = lane; g < u.n_wg; g += 64) {
        const float* a = u.loss_partials + (long)g * 8;
        const float* cc = u.loss_partials + ((long)u.n_wg + g) * 8;
        p0 += a[0]; p3 += a[3]; p4 += a[4]; p7 += a[7]; p2 += cc[2];
    }
    p0 = wave_sum(p0); p2 = wave_sum(p2); p3 = wave_sum(p3); p4 = wave_sum(p4); p7 = wave_sum(p7);
    if (lane == 0) {
        const float n = (float)u.B;
        const float surr = p0 / n, ent = p3 / n, kl = p4 / n, crit = p2 / n;
        float total = surr;
        if (u.entropy_weight != 0.0f) total -= u.entropy_weight * ent;
        if (u.kl_loss_weight > 0.0f) total += u.kl_loss_weight * kl;
        u.totals[0] += (double)surr; u.totals[1] += (double)total; u.totals[2] += (double)crit;
        u.totals[3] += (double)ent; u.totals[4] += (double)kl;
        u.totals[5] += (double)u.loss_partials[5]; u.totals[6] += (double)u.loss_partials[6];
        u.totals[7] += p7 > 0.f ? 1.0 : 0.0;
        u.totals[8] += 1.0;
        // the record of this mini-batch into the other normaliser slot, then the next mini-batch
        const long mb = u.cursor[0];
        float m, v;
        double cnt;
        minibatch_vn_state(u, mb, m, v, cnt);
        const int slot = (int)(mb & 1) ^ 1;
        u.vn_mean[slot] = m; u.vn_var[slot] = v; u.vn_count[slot] = cnt;
        u.cursor[0] = mb + 1;
    }
}

// partials: pairs (actor, critic) of squared-norm partials, added by every wave in the same order; NULL: norm_scratch[0..1]
__global__ __launch_bounds__(256) void lstm_update_adam_kernel(const LstmUpdDev u, const double* partials, const unsigned n_partials) {
    if (blockIdx.x == gridDim.x - 1) { lstm_update_bookkeeping(u); return; }
    double sq[2];
    if (partials) {
        const unsigned lane = threadIdx.x & 63;
        double p0 = 0.0, p1 = 0.0;
        for (unsigned b = lane; b < n_partials; b += 64) { p0 += partials[2 * b]; p1 += partials[2 * b + 1]; }
        sq[0] = wave_sum(p0); sq[1] = wave_sum(p1);
    } else {
        sq[0] = u.norm_scratch[0]; sq[1] = u.norm_scratch[1];
    }
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= u.bucket_total) return;
    const int w = idx >= u.actor_size ? 1 : 0;
    // adam.hip's clip_adam_kernel, expression for expression
    const float total_norm = (float)sqrt(sq[w]);
    float coef = 1.0f;
    if (u.max_norm > 0.f) coef = fminf(u.max_norm / (total_norm + 1e-6f), 1.0f);
    const float gs = u.grad_scale * coef;
    const double t = (double)u.step_counts[w];
    const double bc1 = 1.0 - pow((double)u.beta1, t);
    const double bc2 = 1.0 - pow((double)u.beta2, t);
    const float step_size = (float)((double)u.lr[0] / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    const Pmv s = pmv_load<false>(u.params, u.exp_avg, u.exp_avg_sq, idx, true);
    adam_element(u.params, u.exp_avg, u.exp_avg_sq, u.beta1, u.beta2, u.adam_eps, idx, u.grads[idx], s, gs, step_size, bc2_sqrt);
}

int check_update_shapes(const ppoaf_lstm_update_args_t* a) {
    PPOAF_REQUIRE(a, "lstm_update: null args");
    ppoaf_lstm_desc_t da = a->actor, dc = a->critic;
    da.rows = dc.rows = 1;                         // (`rows` is not read: B rules)
    if (!da.params) da.params = reinterpret_cast<const float*>(a);      // shapes only: never followed
    if (!dc.params) dc.params = reinterpret_cast<const float*>(a);
    if (int rc = check_lstm_desc(&da, false, "lstm_update: actor")) return rc;
    if (int rc = check_lstm_desc(&dc, false, "lstm_update: critic")) return rc;
    PPOAF_REQUIRE(a->actor.hidden == a->critic.hidden,
                  "lstm_update: LSTM hidden sizes differ (actor %d, critic %d): one launch has one block size",
                  a->actor.hidden, a->critic.hidden);
    PPOAF_REQUIRE(a->actor.steps == a->critic.steps, "lstm_update: steps differ (actor %lld, critic %lld)",
                  (long long)a->actor.steps, (long long)a->critic.steps);
    PPOAF_REQUIRE(a->critic.out_dim == 1, "lstm_update: critic out_dim must be 1");
    PPOAF_REQUIRE(a->head_kind == PPOAF_HEAD_CATEGORICAL || a->head_kind == PPOAF_HEAD_GAUSSIAN,
                  "lstm_update: head_kind=%d (0 categorical, 1 Gaussian)", a->head_kind);
    PPOAF_REQUIRE(a->B >= 2 && a->B <= (1L << 20), "lstm_update: B=%lld not in [2, 2^20]", (long long)a->B);
    PPOAF_REQUIRE(a->batch_stride >= a->B, "lstm_update: batch_stride=%lld < B=%lld", (long long)a->batch_stride, (long long)a->B);
    const long lds = upd_lds_bytes(a->actor.hidden);
    PPOAF_REQUIRE(lds <= kLdsCarve, "lstm_update: hidden %d needs %ld bytes of LDS per workgroup, %ld available", a->actor.hidden,
                  lds, kLdsCarve);
    return PPOAF_OK;
}

int check_update_args(const ppoaf_lstm_update_args_t* a) {
    if (int rc = check_update_shapes(a)) return rc;
    PPOAF_REQUIRE(a->params && a->grads && a->exp_avg && a->exp_avg_sq, "lstm_update: params / grads / exp_avg / exp_avg_sq is NULL");
    ppoaf_lstm_desc_t da = a->actor, dc = a->critic;
    da.rows = dc.rows = a->B;
    const long na = layout_of(da).size, nc = layout_of(dc).size;
    const bool gauss = a->head_kind == PPOAF_HEAD_GAUSSIAN;
    PPOAF_REQUIRE(gauss ? a->log_std_offset == na : a->log_std_offset == -1,
                  "lstm_update: log_std_offset=%lld (%ld behind the actor's network, -1 without a Gaussian head)",
                  (long long)a->log_std_offset, na);
    PPOAF_REQUIRE(a->actor_size == na + (gauss ? pad4(a->actor.out_dim) : 0), "lstm_update: actor_size=%lld, the actor's bucket holds %ld",
                  (long long)a->actor_size, na + (gauss ? pad4(a->actor.out_dim) : 0));
    PPOAF_REQUIRE(a->bucket_total == a->actor_size + nc, "lstm_update: bucket_total=%lld, actor + critic hold %ld",
                  (long long)a->bucket_total, (long)a->actor_size + nc);
    PPOAF_REQUIRE(a->actor.params == a->params && a->critic.params == a->params + a->actor_size,
                  "lstm_update: actor.params / critic.params do not point into params");
    PPOAF_REQUIRE(a->actor.grads == a->grads && a->critic.grads == a->grads + a->actor_size,
                  "lstm_update: actor.grads / critic.grads do not point into grads");
    PPOAF_REQUIRE(a->step_counts && a->lr && a->norm_scratch, "lstm_update: step_counts / lr / norm_scratch is NULL");
    PPOAF_REQUIRE(a->obs && a->critic_obs && a->perm && a->row_map, "lstm_update: obs / critic_obs / perm / row_map is NULL");
    PPOAF_REQUIRE(a->actor.steps == 1 || a->terminal, "lstm_update: terminal is NULL with steps > 1");
    PPOAF_REQUIRE(a->n_rows >= a->actor.steps && a->n_rows <= 0x7fffffffL, "lstm_update: n_rows=%lld", (long long)a->n_rows);
    PPOAF_REQUIRE(a->n_items >= 1 && a->n_items <= a->n_rows - a->actor.steps + 1, "lstm_update: n_items=%lld with n_rows=%lld, steps=%lld",
                  (long long)a->n_items, (long long)a->n_rows, (long long)a->actor.steps);
    PPOAF_REQUIRE(a->raw_actions && a->advantages && a->old_log_probs && a->rewards_to_go && a->values,
                  "lstm_update: raw_actions / advantages / old_log_probs / rewards_to_go / values is NULL");
    PPOAF_REQUIRE(a->actor_hidden && a->actor_cell && a->critic_hidden && a->critic_cell, "lstm_update: a hidden-state table is NULL");
    PPOAF_REQUIRE(a->cursor && a->vn_mean && a->vn_var && a->vn_count && a->loss_partials && a->totals,
                  "lstm_update: cursor / vn_mean / vn_var / vn_count / loss_partials / totals is NULL");
    PPOAF_REQUIRE(!a->normalize_values || (a->vn_records && a->n_ranks >= 1), "lstm_update: vn_records missing");
    PPOAF_REQUIRE(!a->normalize_adv || a->adv_records, "lstm_update: adv_records missing");
    const UpdLayout U = upd_layout(*a);
    PPOAF_REQUIRE(a->workspace && a->workspace_floats >= U.total, "lstm_update: workspace holds %lld floats, %ld needed",
                  (long long)a->workspace_floats, U.total);
    return PPOAF_OK;
}

int n_wgrad_tiles(const ppoaf_lstm_update_args_t* a, UpdJobs* Jout, const LstmUpdDev* u);

long norm_doubles(const ppoaf_lstm_update_args_t* a) {
    const long tiles = n_wgrad_tiles(a, nullptr, nullptr), blocks = (a->bucket_total + 255) / 256;
    return 2 + 2 * (tiles > blocks ? tiles : blocks);
}

int make_dev(const ppoaf_lstm_update_args_t* a, LstmUpdDev& u) {
    if (int rc = check_update_args(a)) return rc;
    PPOAF_REQUIRE(a->norm_scratch_doubles >= norm_doubles(a), "lstm_update: norm_scratch holds %lld doubles, %ld needed",
                  (long long)a->norm_scratch_doubles, norm_doubles(a));
    u = LstmUpdDev{};
    const UpdLayout U = upd_layout(*a);
    float* ws = a->workspace;
    for (int w = 0; w < 2; ++w) {
        ppoaf_lstm_desc_t d = w == 0 ? a->actor : a->critic;
        d.rows = a->B;
        LstmArgs& n = u.net[w];
        n = lstm_args_of(&d);
        const UpdWs& p = U.w[w];
        n.ws = ws + p.net;
        n.x = u.xs[w] = ws + p.x;
        n.h0 = u.h0s[w] = ws + p.h0;
        n.c0 = u.c0s[w] = ws + p.c0;
        n.hn = ws + p.hn; n.cn = ws + p.cn;
        n.dout = u.douts[w] = ws + p.dout;
        n.stash = 1;
    }
    u.dls = ws + U.w[0].dls;
    u.H = a->actor.hidden;
    u.obs[0] = a->obs; u.obs[1] = a->critic_obs;
    u.tab_h[0] = a->actor_hidden; u.tab_c[0] = a->actor_cell; u.tab_h[1] = a->critic_hidden; u.tab_c[1] = a->critic_cell;
    u.terminal = a->actor.steps > 1 ? a->terminal : nullptr;
    u.perm = a->perm; u.row_map = a->row_map; u.n_rows = a->n_rows; u.n_items = a->n_items;
    u.raw_actions = a->raw_actions; u.adv = a->advantages; u.old_lp = a->old_log_probs; u.rtg = a->rewards_to_go;
    u.values = a->values;
    u.cursor = a->cursor; u.B = a->B; u.batch_stride = a->batch_stride;
    u.normalize_values = a->normalize_values; u.n_ranks = a->n_ranks;
    u.vn_mean = a->vn_mean; u.vn_var = a->vn_var; u.vn_count = a->vn_count; u.vn_records = a->vn_records;
    u.adv_records = a->adv_records;
    u.normalize_adv = a->normalize_adv; u.use_huber = a->use_huber; u.head_kind = a->head_kind;
    u.surr_clip = a->surr_clip; u.entropy_weight = a->entropy_weight; u.kl_loss_weight = a->kl_loss_weight;
    u.huber_delta = a->huber_delta; u.min_std = a->min_std;
    u.log_std = a->log_std_offset >= 0 ? a->params + a->log_std_offset : nullptr;
    u.loss_partials = a->loss_partials; u.totals = a->totals;
    u.n_wg = (int)((a->B + kLRows - 1) / kLRows);
    u.params = a->params; u.grads = a->grads; u.exp_avg = a->exp_avg; u.exp_avg_sq = a->exp_avg_sq;
    u.bucket_total = a->bucket_total; u.actor_size = a->actor_size;
    u.step_counts = a->step_counts; u.lr = a->lr; u.norm_scratch = a->norm_scratch;
    u.beta1 = a->beta1; u.beta2 = a->beta2; u.adam_eps = a->adam_eps; u.grad_scale = a->grad_scale; u.max_norm = a->max_norm;
    return PPOAF_OK;
}

// the jobs of both networks (K18's list each; the actor's log_std behind its own); Jout / u may be NULL: the count alone
int n_wgrad_tiles(const ppoaf_lstm_update_args_t* a, UpdJobs* Jout, const LstmUpdDev* u) {
    UpdJobs J{};
    LstmUpdDev z{};
    if (!u) {
        for (int w = 0; w < 2; ++w) {
            ppoaf_lstm_desc_t d = w == 0 ? a->actor : a->critic;
            d.rows = a->B;
            ppoaf_lstm_desc_t dd = d;
            dd.params = reinterpret_cast<const float*>(a);
            z.net[w] = lstm_args_of(&dd);
        }
        u = &z;
    }
    int nt = 0;
    for (int w = 0; w < 2; ++w) {
        if (w == 1) J.first_critic_tile = nt;
        float* G = w == 0 ? a->grads : a->grads + a->actor_size;
        nt = lstm_wgrad_add_jobs(J.j, J.n, nt, u->net[w], a->actor.hidden, u->xs[w], u->h0s[w], G);
        if (w == 0 && a->head_kind == PPOAF_HEAD_GAUSSIAN) {
            WJob& jb = J.j[J.n++];
            jb = WJob{};
            jb.A = u->dls; jb.lda = 8; jb.B = nullptr; jb.ldb = 0; jb.M = 1; jb.Nc = a->actor.out_dim; jb.mode = kBDiag;
            jb.K = a->B; jb.out = a->grads + (a->log_std_offset >= 0 ? a->log_std_offset : 0); jb.ldo = 1; jb.S = (int)a->actor.steps;
            jb.tiles_n = 1; jb.tile_begin = nt;
            nt += 1;
        }
    }
    J.n_tiles = nt;
    if (Jout) *Jout = J;
    return nt;
}

template <int H>
int launch_fwd_bwd(const LstmUpdDev& u, hipStream_t s) {
    hipLaunchKernelGGL(lstm_update_fwd_bwd_kernel<H>, dim3(2u * (unsigned)u.n_wg), dim3(H / 16 * 64), 0, s, u);
    return check_launch("lstm_update_fwd_bwd");
}

}  // namespace
}  // namespace ppoaf

using namespace ppoaf;

// the layout the ctypes structure of _lib.py restates (tests/test_lstm_update_abi.py reads this list)
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, actor, 0);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, critic, 72);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, params, 144);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, grads, 152);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, exp_avg, 160);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, exp_avg_sq, 168);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, bucket_total, 176);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, actor_size, 184);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, log_std_offset, 192);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, step_counts, 200);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, lr, 208);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, norm_scratch, 216);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, norm_scratch_doubles, 224);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, beta1, 232);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, beta2, 236);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, adam_eps, 240);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, grad_scale, 244);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, max_norm, 248);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, head_kind, 252);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, obs, 256);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, critic_obs, 264);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, terminal, 272);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, perm, 280);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, row_map, 288);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, n_rows, 296);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, n_items, 304);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, raw_actions, 312);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, advantages, 320);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, old_log_probs, 328);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, rewards_to_go, 336);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, values, 344);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, actor_hidden, 352);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, actor_cell, 360);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, critic_hidden, 368);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, critic_cell, 376);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, cursor, 384);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, B, 392);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, batch_stride, 400);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, normalize_values, 408);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, n_ranks, 412);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, vn_mean, 416);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, vn_var, 424);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, vn_count, 432);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, vn_records, 440);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, adv_records, 448);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, normalize_adv, 456);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, use_huber, 460);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, surr_clip, 464);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, entropy_weight, 468);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, kl_loss_weight, 472);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, huber_delta, 476);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, min_std, 480);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, _pad, 484);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, loss_partials, 488);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, totals, 496);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, workspace, 504);
PPOAF_LAYOUT(ppoaf_lstm_update_args_t, workspace_floats, 512);
static_assert(sizeof(ppoaf_lstm_update_args_t) == 520, "ppoaf_lstm_update_args_t");

extern "C" int ppoaf_lstm_update_check(const ppoaf_lstm_update_args_t* a, int32_t pointers) {
    return pointers ? check_update_args(a) : check_update_shapes(a);
}

extern "C" int ppoaf_lstm_update_workspace_floats(const ppoaf_lstm_update_args_t* a, int64_t* out) {
    if (int rc = check_update_shapes(a)) return rc;
    PPOAF_REQUIRE(out != nullptr, "lstm_update_workspace_floats: out is NULL");
    PPOAF_REQUIRE(a->bucket_total >= 1 && a->actor_size >= 1 && a->actor_size < a->bucket_total,
                  "lstm_update_workspace_floats: bucket_total=%lld, actor_size=%lld", (long long)a->bucket_total, (long long)a->actor_size);
    out[0] = upd_layout(*a).total;
    out[1] = norm_doubles(a);
    out[2] = upd_lds_bytes(a->actor.hidden);
    return PPOAF_OK;
}

extern "C" int ppoaf_lstm_update_fwd_bwd(const ppoaf_lstm_update_args_t* a, ppoaf_stream_t stream) {
    LstmUpdDev u;
    if (int rc = make_dev(a, u)) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (u.H) {
        case 32: return launch_fwd_bwd<32>(u, s);
        case 64: return launch_fwd_bwd<64>(u, s);
    }
    return launch_fwd_bwd<128>(u, s);
}

extern "C" int ppoaf_lstm_update_wgrad(const ppoaf_lstm_update_args_t* a, ppoaf_stream_t stream) {
    LstmUpdDev u;
    if (int rc = make_dev(a, u)) return rc;
    UpdJobs J;
    const int nt = n_wgrad_tiles(a, &J, &u);
    hipLaunchKernelGGL(lstm_update_wgrad_kernel, dim3((unsigned)nt + 1u), dim3(256), 0, (hipStream_t)stream, J, u.grad_scale, u.step_counts,
                       u.norm_scratch);
    return check_launch("lstm_update_wgrad");
}

extern "C" int ppoaf_lstm_update_adam(const ppoaf_lstm_update_args_t* a, int32_t norm_mode, ppoaf_stream_t stream) {
    LstmUpdDev u;
    if (int rc = make_dev(a, u)) return rc;
    PPOAF_REQUIRE(norm_mode >= 0 && norm_mode <= 2, "lstm_update_adam: norm_mode=%d (0 .. 2)", norm_mode);
    const unsigned blocks = (unsigned)((u.bucket_total + 255) / 256);
    unsigned n_partials = (unsigned)n_wgrad_tiles(a, nullptr, &u);
    if (norm_mode == 1) {
        hipLaunchKernelGGL(lstm_update_sqnorm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, u);
        if (int rc = check_launch("lstm_update_adam/sqnorm")) return rc;
        n_partials = blocks;
    }
    hipLaunchKernelGGL(lstm_update_adam_kernel, dim3(blocks + 1u), dim3(256), 0, (hipStream_t)stream, u,
                       norm_mode == 2 ? (const double*)nullptr : (const double*)(u.norm_scratch + 2), n_partials);
    return check_launch("lstm_update_adam");
}
