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

#include "lstm_update_device.hpp"

namespace ppoaf {
namespace {

constexpr int kUpdMaxJobs = 2 * kLMaxJobs;

// per-network pieces of the workspace, float offsets: K18's stash, then what the prologue stages and the head leaves
struct UpdWs { long net, x, h0, c0, hn, cn, dout, dls, end; };

struct UpdLayout { UpdWs w[2]; long total; };

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
    return 4 * (fwd + (b1 > b2 ? b1 : b2) + kUpdHeadLds);
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

    // (The prologue, the window staging and the d out hand-over below are restated in lstm_stacked_update.hip --
    // lstm_update_prologue, lstm_update_stage_windows, lstm_update_leave_dout: a change to the perm / row_map / terminal
    // rule here goes there too.)
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
    lstm_update_wgrad_block(J, grad_scale, step_counts, norm_scratch);
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

int check_update_shapes(const ppoaf_lstm_update_args_t* a) {
    PPOAF_REQUIRE(a, "lstm_update: null args");
    ppoaf_lstm_desc_t da = a->actor, dc = a->critic;
    da.rows = dc.rows = 1;                         // (`rows` is not read: B rules)
    if (!da.params) da.params = reinterpret_cast<const float*>(a);      // shapes only: never followed
    if (!dc.params) dc.params = reinterpret_cast<const float*>(a);
    if (int rc = check_lstm_desc(&da, false, "lstm_update: actor")) return rc;
    if (int rc = check_lstm_desc(&dc, false, "lstm_update: critic")) return rc;
    if (int rc = check_update_pair(a, "lstm_update")) return rc;
    const long lds = upd_lds_bytes(a->actor.hidden);
    PPOAF_REQUIRE(lds <= kLdsCarve, "lstm_update: hidden %d needs %ld bytes of LDS per workgroup, %ld available", a->actor.hidden,
                  lds, kLdsCarve);
    return PPOAF_OK;
}

int check_update_args(const ppoaf_lstm_update_args_t* a) {
    if (int rc = check_update_shapes(a)) return rc;
    ppoaf_lstm_desc_t da = a->actor, dc = a->critic;
    da.rows = dc.rows = a->B;
    if (int rc = check_update_pointers(a, layout_of(da).size, layout_of(dc).size, "lstm_update")) return rc;
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
    fill_update_dev(a, u);
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
    unsigned n_partials = (unsigned)n_wgrad_tiles(a, nullptr, &u);
    if (norm_mode == 1) {
        const unsigned blocks = (unsigned)((u.bucket_total + 255) / 256);
        hipLaunchKernelGGL(lstm_update_sqnorm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, u);
        if (int rc = check_launch("lstm_update_adam/sqnorm")) return rc;
        n_partials = blocks;
    }
    return launch_update_adam(u, norm_mode == 2 ? (const double*)nullptr : (const double*)(u.norm_scratch + 2), n_partials,
                              (hipStream_t)stream, "lstm_update_adam");
}
