// What the fused LSTM update epochs share: K22 (lstm_update.hip, one LSTM layer per network) and K22 for two stacked
// layers (lstm_stacked_update.hip).  The device arguments of a mini-batch, a workgroup of the weight-gradient launch, the
// closing launch -- clip norm + Adam, totals, normaliser record, cursor -- and the host checks of what the two argument
// structures have in common: one copy of each.  The tile kernels, with their recurrent bodies and the layout of the
// hidden tables, are each file's own.
#pragma once
#include "lstm_device.hpp"
#include "ppo_update_dev.hpp"
#include "running_stats_device.hpp"

namespace ppoaf {
namespace {

constexpr long kLdsCarve = 160 * 1024;             // LDS a gfx950 workgroup can be given

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

// LDS of a tile's prologue and head, floats: sWin, sRow, sRowF, sMisc, sActF, sOut, sDOut of the kernels below
constexpr long kUpdHeadLds = kLRows * 16 + kLRows + 48 + 4 + kLRows * 8 + 2 * kLRows * kMaxOut;

// One workgroup of the weight-gradient launch over a job table (Jobs: WJob j[]; n, first_critic_tile, n_tiles): its tile
// STORED into the bucket, its pair of squared-norm partials; the workgroup behind the last tile advances the Adam step
// counters of the step that follows.
template <class Jobs>
__device__ __forceinline__ void lstm_update_wgrad_block(const Jobs& J, const float grad_scale, int64_t* step_counts, double* norm_scratch) {
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

// host: the closing launch over the squared-norm partials norm_scratch[2 ..] (pairs, n_partials of them)
inline int launch_update_adam(const LstmUpdDev& u, const double* partials, const unsigned n_partials, hipStream_t s, const char* what) {
    const unsigned blocks = (unsigned)((u.bucket_total + 255) / 256);
    hipLaunchKernelGGL(lstm_update_adam_kernel, dim3(blocks + 1u), dim3(256), 0, s, u, partials, n_partials);
    return check_launch(what);
}

// host: what both argument structures ask of the pair of networks and of the batch
template <class A>
int check_update_pair(const A* a, const char* what) {
    PPOAF_REQUIRE(a->actor.hidden == a->critic.hidden,
                  "%s: LSTM hidden sizes differ (actor %d, critic %d): one launch has one block size", what,
                  a->actor.hidden, a->critic.hidden);
    PPOAF_REQUIRE(a->actor.steps == a->critic.steps, "%s: steps differ (actor %lld, critic %lld)", what,
                  (long long)a->actor.steps, (long long)a->critic.steps);
    PPOAF_REQUIRE(a->critic.out_dim == 1, "%s: critic out_dim must be 1", what);
    PPOAF_REQUIRE(a->head_kind == PPOAF_HEAD_CATEGORICAL || a->head_kind == PPOAF_HEAD_GAUSSIAN,
                  "%s: head_kind=%d (0 categorical, 1 Gaussian)", what, a->head_kind);
    PPOAF_REQUIRE(a->B >= 2 && a->B <= (1L << 20), "%s: B=%lld not in [2, 2^20]", what, (long long)a->B);
    PPOAF_REQUIRE(a->batch_stride >= a->B, "%s: batch_stride=%lld < B=%lld", what, (long long)a->batch_stride, (long long)a->B);
    return PPOAF_OK;
}

// host: the pointer checks both argument structures share (A: ppoaf_lstm_update_args_t / ppoaf_lstm2_update_args_t); na, nc:
// the floats of the actor's and the critic's network in the bucket
template <class A>
int check_update_pointers(const A* a, const long na, const long nc, const char* what) {
    PPOAF_REQUIRE(a->params && a->grads && a->exp_avg && a->exp_avg_sq, "%s: params / grads / exp_avg / exp_avg_sq is NULL", what);
    const bool gauss = a->head_kind == PPOAF_HEAD_GAUSSIAN;
    PPOAF_REQUIRE(gauss ? a->log_std_offset == na : a->log_std_offset == -1,
                  "%s: log_std_offset=%lld (%ld behind the actor's network, -1 without a Gaussian head)", what,
                  (long long)a->log_std_offset, na);
    PPOAF_REQUIRE(a->actor_size == na + (gauss ? pad4(a->actor.out_dim) : 0), "%s: actor_size=%lld, the actor's bucket holds %ld", what,
                  (long long)a->actor_size, na + (gauss ? pad4(a->actor.out_dim) : 0));
    PPOAF_REQUIRE(a->bucket_total == a->actor_size + nc, "%s: bucket_total=%lld, actor + critic hold %ld", what,
                  (long long)a->bucket_total, (long)a->actor_size + nc);
    PPOAF_REQUIRE(a->actor.params == a->params && a->critic.params == a->params + a->actor_size,
                  "%s: actor.params / critic.params do not point into params", what);
    PPOAF_REQUIRE(a->actor.grads == a->grads && a->critic.grads == a->grads + a->actor_size,
                  "%s: actor.grads / critic.grads do not point into grads", what);
    PPOAF_REQUIRE(a->step_counts && a->lr && a->norm_scratch, "%s: step_counts / lr / norm_scratch is NULL", what);
    PPOAF_REQUIRE(a->obs && a->critic_obs && a->perm && a->row_map, "%s: obs / critic_obs / perm / row_map is NULL", what);
    PPOAF_REQUIRE(a->actor.steps == 1 || a->terminal, "%s: terminal is NULL with steps > 1", what);
    PPOAF_REQUIRE(a->n_rows >= a->actor.steps && a->n_rows <= 0x7fffffffL, "%s: n_rows=%lld", what, (long long)a->n_rows);
    PPOAF_REQUIRE(a->n_items >= 1 && a->n_items <= a->n_rows - a->actor.steps + 1, "%s: n_items=%lld with n_rows=%lld, steps=%lld", what,
                  (long long)a->n_items, (long long)a->n_rows, (long long)a->actor.steps);
    PPOAF_REQUIRE(a->raw_actions && a->advantages && a->old_log_probs && a->rewards_to_go && a->values,
                  "%s: raw_actions / advantages / old_log_probs / rewards_to_go / values is NULL", what);
    PPOAF_REQUIRE(a->actor_hidden && a->actor_cell && a->critic_hidden && a->critic_cell, "%s: a hidden-state table is NULL", what);
    PPOAF_REQUIRE(a->cursor && a->vn_mean && a->vn_var && a->vn_count && a->loss_partials && a->totals,
                  "%s: cursor / vn_mean / vn_var / vn_count / loss_partials / totals is NULL", what);
    PPOAF_REQUIRE(!a->normalize_values || (a->vn_records && a->n_ranks >= 1), "%s: vn_records missing", what);
    PPOAF_REQUIRE(!a->normalize_adv || a->adv_records, "%s: adv_records missing", what);
    return PPOAF_OK;
}

// host: every field of `u` that does not depend on the networks' layout
template <class A>
void fill_update_dev(const A* a, LstmUpdDev& u) {
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
}

}  // namespace
}  // namespace ppoaf
