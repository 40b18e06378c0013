// K22 for two stacked LSTM layers: one mini-batch of the PPO update of a two-layer LSTM actor / critic pair as four
// launches that read the device cursor -- a whole epoch is enqueued without returning to the host and replayed from
// hipGraphs.  What K22 (lstm_update.hip) does in three launches, over the stacked bodies of lstm_stacked_device.hpp:
//   forward   2 * ceil(B/16) workgroups (actor tiles, then critic tiles) of 2 H / 16 waves.  K22's prologue: the tile's 16
//             items of the shuffled permutation -> their observation windows (buffer rows row_map[item + s]; actor
//             observations zeroed strictly after a terminal position) and the stored state of the LAST position, here
//             both layers' (h, c) from the buffer's [rows, 2, H] tables, staged into the workspace as [B, 2, H].  Then
//             the wavefront forward body with the stash on, the final (h, c) of both layers back to the table rows,
//             and K12's head + loss terms on one wave (ppo_head_loss); d loss / d out stays in the workspace.
//   backward  the same grid with H / 16 waves: the stacked backward body on the tile's rows of the workspace.
//   wgrad     the stacked weight-gradient jobs of both networks (and a Gaussian head's log_std), STORED into the
//             policy's gradient bucket, a pair of squared-norm partials per workgroup; the workgroup behind the last tile
//             advances the Adam step counters.
//   adam      K22's closing launch (lstm_update_device.hpp): clip norms, Adam, totals, normaliser record, cursor.
// Forward and backward are two launches because their workgroups differ: 2 H / 16 waves (16 at H = 128: 128 registers a
// lane) against H / 16 waves with up to 226 registers; one kernel under the 1024-thread bound would put the backward's
// resident W^T slices into the private segment.  Nothing crosses workgroups in either, so the split costs a launch
// boundary and no synchronisation.  No launch waits for another workgroup; none is a memset.
// The tile helpers below restate the prologue, the window staging and the d out hand-over of K22's fwd_bwd kernel: called
// from that kernel they changed its register allocation, and K22's device code is to stay what it is.
#include <cstddef>

#include "lstm_stacked_device.hpp"
#include "lstm_update_device.hpp"

namespace ppoaf {
namespace {

// the forward launch's arguments: K22's (its one-layer `net` is not read) and the two stacked networks
struct Lstm2UpdDev {
    LstmUpdDev u;
    Lstm2Args net[2];                              // actor, critic (x / h0 / c0 / hn / cn / dout: the staged copies)
};
struct Lstm2UpdBwd {
    Lstm2Args net[2];
    int n_wg;
};
struct Upd2Jobs {
    WJob j[2 * kL2MaxJobs];
    int n, first_critic_tile, n_tiles;
};
// kernel arguments travel by value: 4 KiB is what a launch can carry
static_assert(sizeof(Lstm2UpdDev) <= 4096 && sizeof(Lstm2UpdBwd) <= 4096, "update arguments exceed the kernel-argument limit");
static_assert(sizeof(Upd2Jobs) + sizeof(float) + 2 * sizeof(void*) <= 4096, "job table exceeds the kernel-argument limit");

// per-network pieces of the workspace, float offsets: the stacked stash, then what the prologue stages ([B, 2, H] states)
// and the head leaves
struct Upd2Ws { long net, x, h0, c0, hn, cn, dout, dls; };
struct Upd2Layout { Upd2Ws w[2]; long total; };

inline ppoaf_lstm2_desc_t upd2_desc(const ppoaf_lstm2_update_args_t& a, const int w) {
    ppoaf_lstm2_desc_t d = w == 0 ? a.actor : a.critic;
    d.rows = a.B;
    d.state_row_stride = 2L * d.hidden;            // the staged states: [B, 2, H]
    d.state_layer_stride = d.hidden;
    return d;
}

inline Upd2Layout upd2_layout(const ppoaf_lstm2_update_args_t& a) {
    Upd2Layout U{};
    long o = 0;
    for (int w = 0; w < 2; ++w) {
        const ppoaf_lstm2_desc_t d = upd2_desc(a, w);
        const long B = a.B, S = d.steps, H = d.hidden;
        Upd2Ws& p = U.w[w];
        p.net = o; o += pad4(layout2_of(d).total);
        p.x = o; o += pad4(B * S * d.in_dim);
        p.h0 = o; o += B * 2 * H;
        p.c0 = o; o += B * 2 * H;
        p.hn = o; o += B * 2 * H;
        p.cn = o; o += B * 2 * H;
        p.dout = o; o += pad4(B * d.out_dim);
        p.dls = o; o += w == 0 ? B * 8 : 0;
    }
    U.total = o;
    return U;
}

// static LDS of a forward workgroup: the forward body's x buffers and the two layers' double-buffered h tiles, beside the
// prologue / head arrays -- 46352 / 54544 / 70928 bytes at H = 32 / 64 / 128.  (The backward launch holds the backward
// body's 19200 / 33280 / 66048 alone.)
inline long upd2_lds_bytes(const int H) {
    const long HS = H + 4, XS = kLMaxIn + 4;
    return 4 * (2 * kLRows * XS + 4 * kLRows * HS + kUpdHeadLds);
}

// The tile's 16 items of mini-batch `mb`, their windows' buffer rows (sWin; -1: zeros), the row of the last position
// (sRow; -1: dead row) and its scalars (sRowF, sActF), and the mini-batch's moments (sMisc).  No barrier inside.
// (This and the two helpers below restate lstm_update_fwd_bwd_kernel's text in lstm_update.hip: keep the two in step.)
__device__ __forceinline__ void lstm_update_prologue(const LstmUpdDev& u, const int which, const long r0, const int S, const int O,
                                                     const long mb, int* sWin, int* sRow, float* sRowF, float* sMisc, float* sActF) {
    const int tid = threadIdx.x;
    const long B = u.B;
    const long base = mb * u.batch_stride;
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
}

// the tile's windows into its rows of the workspace (the weight-gradient launch reads them too)
template <int NT>
__device__ __forceinline__ void lstm_update_stage_windows(const LstmUpdDev& u, const int which, const long r0, const int S, const int I,
                                                          const int* sWin) {
    const int tid = threadIdx.x;
    const float* obs = u.obs[which];
    float* xs = u.xs[which];
    const int SI = S * I;
    for (int e = tid; e < kLRows * SI; e += NT) {
        const int r = e / SI, rem = e - r * SI, s = rem / I, k = rem - s * I;
        const long n = r0 + r;
        if (n < u.B) {
            const int wr = sWin[r * 16 + s];
            xs[(n * S + s) * I + k] = wr >= 0 ? obs[(long)wr * I + k] : 0.f;
        }
    }
}

// d loss / d out of the tile's rows (and a Gaussian head's per-row d loss / d log_std) where the backward and the
// weight-gradient launch read them
template <int NT>
__device__ __forceinline__ void lstm_update_leave_dout(const LstmUpdDev& u, const int which, const long r0, const int O, const int* sRow,
                                                       const float* sOut, const float* sDOut) {
    const int tid = threadIdx.x;
    for (int e = tid; e < kLRows * O; e += NT) {
        const int r = e / O, o = e - r * O;
        const long n = r0 + r;
        if (n < u.B) u.douts[which][n * O + o] = sDOut[r * kMaxOut + o];
    }
    if (which == 0 && u.head_kind == PPOAF_HEAD_GAUSSIAN) {
        for (int e = tid; e < kLRows * 8; e += NT) {
            const int r = e >> 3, d = e & 7;
            const long n = r0 + r;
            if (n < u.B) u.dls[n * 8 + d] = (d < O && sRow[r] >= 0) ? sOut[r * kMaxOut + 8 + d] : 0.f;
        }
    }
}

template <int H>
__global__ __launch_bounds__(2 * (H / 16) * 64) PPOAF_NO_PK_F32 void lstm2_update_forward_kernel(const Lstm2UpdDev v) {
    constexpr int NT = 2 * (H / 16) * 64, H2 = 2 * H;
    __shared__ int sWin[kLRows * 16];              // buffer row of (tile row, step); -1: zeros
    __shared__ int sRow[kLRows];                   // buffer row of the item's last position; -1: dead row
    __shared__ float sRowF[48];
    __shared__ float sMisc[4];
    __shared__ float sActF[kLRows * 8];
    __shared__ float sOut[kLRows * kMaxOut];
    __shared__ float sDOut[kLRows * kMaxOut];
    const LstmUpdDev& u = v.u;
    const int tid = threadIdx.x;
    const int which = (int)blockIdx.x >= u.n_wg ? 1 : 0;
    const int g = (int)blockIdx.x - which * u.n_wg;
    const Lstm2Args& a = v.net[which];
    const long B = u.B, r0 = (long)g * kLRows;
    const int S = a.S, I = a.I, O = a.O;
    const long mb = u.cursor[0];

    lstm_update_prologue(u, which, r0, S, O, mb, sWin, sRow, sRowF, sMisc, sActF);
    __syncthreads();

    // ---- the windows and both layers' (h0, c0) -- a table row is [2, H], so is a staged row -- into this tile's rows of
    //      the workspace
    lstm_update_stage_windows<NT>(u, which, r0, S, I, sWin);
    {
        const float* th = u.tab_h[which];
        const float* tc = u.tab_c[which];
        for (int e = tid; e < kLRows * H2; e += NT) {
            const int r = e / H2, k = e - r * H2;
            const long n = r0 + r;
            if (n < B) {
                const int row = sRow[r];
                u.h0s[which][n * H2 + k] = row >= 0 ? th[(long)row * H2 + k] : 0.f;
                u.c0s[which][n * H2 + k] = row >= 0 ? tc[(long)row * H2 + k] : 0.f;
            }
        }
    }
    __syncthreads();                               // (a workgroup reads back only what it wrote itself)

    const float* fo = lstm2_rows_forward<H, true>(a, (unsigned)g);

    // ---- the final (h, c) of both layers replace the stored ones (rows of a mini-batch are distinct; this tile read its
    //      own above)
    for (int e = tid; e < kLRows * H2; e += NT) {
        const int r = e / H2, k = e - r * H2;
        const long n = r0 + r;
        if (n < B && sRow[r] >= 0) {
            const long at = (long)sRow[r] * H2 + k;
            u.tab_h[which][at] = a.hn[n * H2 + k];
            u.tab_c[which][at] = a.cn[n * H2 + k];
        }
    }
    for (int e = tid; e < kLRows * kMaxOut; e += NT) {
        const int r = e / kMaxOut, k = e - r * kMaxOut;
        sOut[e] = k < O ? fo[r * kLFS + k] : 0.f;
    }
    __syncthreads();

    // ---- head + loss of the 16 rows by one wave (K12's), d loss / d out -> sDOut -> the workspace
    if (tid < 64) ppo_head_loss(u, which, g, O, u.log_std, sRow, sRowF, sMisc, sActF, sOut, sDOut, tid, B);
    __syncthreads();
    lstm_update_leave_dout<NT>(u, which, r0, O, sRow, sOut, sDOut);
}

template <int H>
__global__ __launch_bounds__(H / 16 * 64) PPOAF_NO_PK_F32 void lstm2_update_backward_kernel(const Lstm2UpdBwd v) {
    const int which = (int)blockIdx.x >= v.n_wg ? 1 : 0;
    lstm2_rows_backward<H>(v.net[which], (unsigned)((int)blockIdx.x - which * v.n_wg));
}

__global__ __launch_bounds__(256) PPOAF_NO_PK_F32 void lstm2_update_wgrad_kernel(const Upd2Jobs J, const float grad_scale,
                                                                                  int64_t* step_counts, double* norm_scratch) {
    lstm_update_wgrad_block(J, grad_scale, step_counts, norm_scratch);
}

int check_update2_shapes(const ppoaf_lstm2_update_args_t* a) {
    PPOAF_REQUIRE(a, "lstm2_update: null args");
    for (int w = 0; w < 2; ++w) {
        ppoaf_lstm2_desc_t d = w == 0 ? a->actor : a->critic;
        const long H = d.hidden;
        PPOAF_REQUIRE(d.state_row_stride == 2 * H && d.state_layer_stride == H,
                      "lstm2_update: %s: state strides (row %lld, layer %lld) are not the hidden tables' [rows, 2, %ld]",
                      w == 0 ? "actor" : "critic", (long long)d.state_row_stride, (long long)d.state_layer_stride, H);
        d.rows = 1;                                // (`rows` is not read: B rules)
        if (!d.params) d.params = reinterpret_cast<const float*>(a);     // shapes only: never followed
        if (int rc = check_lstm2_desc(&d, false, w == 0 ? "lstm2_update: actor" : "lstm2_update: critic")) return rc;
    }
    if (int rc = check_update_pair(a, "lstm2_update")) return rc;
    const long lds = upd2_lds_bytes(a->actor.hidden);
    PPOAF_REQUIRE(lds <= kLdsCarve, "lstm2_update: hidden %d needs %ld bytes of LDS per workgroup, %ld available", a->actor.hidden,
                  lds, kLdsCarve);
    return PPOAF_OK;
}

int check_update2_args(const ppoaf_lstm2_update_args_t* a) {
    if (int rc = check_update2_shapes(a)) return rc;
    if (int rc = check_update_pointers(a, layout2_of(upd2_desc(*a, 0)).size, layout2_of(upd2_desc(*a, 1)).size, "lstm2_update")) return rc;
    const Upd2Layout U = upd2_layout(*a);
    PPOAF_REQUIRE(a->workspace && a->workspace_floats >= U.total, "lstm2_update: workspace holds %lld floats, %ld needed",
                  (long long)a->workspace_floats, U.total);
    return PPOAF_OK;
}

// the stacked networks over the staged copies; ws == NULL: the shapes alone (what the tile count needs)
void upd2_nets(const ppoaf_lstm2_update_args_t* a, Lstm2Args (&net)[2], LstmUpdDev& u) {
    const Upd2Layout U = upd2_layout(*a);
    float* ws = a->workspace;
    for (int w = 0; w < 2; ++w) {
        const ppoaf_lstm2_desc_t d = upd2_desc(*a, w);
        Lstm2Args& n = net[w];
        n = lstm2_args_of(&d);
        const Upd2Ws& p = U.w[w];
        n.ws = ws + p.net;
        n.x = u.xs[w] = ws + p.x;
        n.h0 = u.h0s[w] = ws + p.h0;
        n.c0 = u.c0s[w] = ws + p.c0;
        n.hn = ws + p.hn; n.cn = ws + p.cn;
        n.dout = u.douts[w] = ws + p.dout;
        n.stash = 1;
    }
    u.dls = ws + U.w[0].dls;
}

// the jobs of both networks (the stacked list each; the actor's log_std behind its own); returns the tile count, or -1
// when two jobs would write one bucket element (each element belongs to exactly one tile: the tiles store, nothing adds)
int upd2_wgrad_jobs(const ppoaf_lstm2_update_args_t* a, Upd2Jobs& J) {
    J = Upd2Jobs{};
    Lstm2Args net[2];
    LstmUpdDev u{};
    upd2_nets(a, net, u);
    int nt = 0;
    for (int w = 0; w < 2; ++w) {
        if (w == 1) J.first_critic_tile = nt;
        float* G = w == 0 ? a->grads : a->grads + a->actor_size;
        nt = lstm2_wgrad_add_jobs(J.j, J.n, nt, net[w], a->actor.hidden, u.xs[w], G);
        if (w == 0 && a->head_kind == PPOAF_HEAD_GAUSSIAN) {
            WJob& jb = J.j[J.n++];
            jb = WJob{};
            jb.A = u.dls; jb.lda = 8; jb.M = 1; jb.Nc = a->actor.out_dim; jb.mode = kBDiag;
            // (log_std lies behind the actor's network: check_update_pointers holds log_std_offset to that)
            jb.K = a->B; jb.out = a->grads + layout2_of(upd2_desc(*a, 0)).size; jb.ldo = 1; jb.S = (int)a->actor.steps;
            jb.tiles_n = 1; jb.tile_begin = nt;
            nt += 1;
        }
    }
    J.n_tiles = nt;
    // every destination (b_ih / b_hh of a layer are one job's out and out2) is a range of its own
    const float* lo[4 * kL2MaxJobs];
    const float* hi[4 * kL2MaxJobs];
    int nr = 0;
    for (int i = 0; i < J.n; ++i) {
        const WJob& jb = J.j[i];
        const long len = jb.mode == kBDiag ? jb.Nc : (long)(jb.M - 1) * jb.ldo + jb.Nc;
        lo[nr] = jb.out; hi[nr++] = jb.out + len;
        if (jb.out2) { lo[nr] = jb.out2; hi[nr++] = jb.out2 + len; }
    }
    for (int i = 0; i < nr; ++i)
        for (int k = i + 1; k < nr; ++k)
            if (lo[i] < hi[k] && lo[k] < hi[i]) return -1;
    return nt;
}

long norm2_doubles(const ppoaf_lstm2_update_args_t* a) {
    Upd2Jobs J;
    const long tiles = upd2_wgrad_jobs(a, J), blocks = (a->bucket_total + 255) / 256;
    return 2 + 2 * (tiles > blocks ? tiles : blocks);
}

int make_dev2(const ppoaf_lstm2_update_args_t* a, Lstm2UpdDev& v) {
    if (int rc = check_update2_args(a)) return rc;
    PPOAF_REQUIRE(a->norm_scratch_doubles >= norm2_doubles(a), "lstm2_update: norm_scratch holds %lld doubles, %ld needed",
                  (long long)a->norm_scratch_doubles, norm2_doubles(a));
    v = Lstm2UpdDev{};
    upd2_nets(a, v.net, v.u);
    fill_update_dev(a, v.u);
    return PPOAF_OK;
}

template <int H>
int launch_update_forward(const Lstm2UpdDev& v, hipStream_t s) {
    hipLaunchKernelGGL(lstm2_update_forward_kernel<H>, dim3(2u * (unsigned)v.u.n_wg), dim3(2 * (H / 16) * 64), 0, s, v);
    return check_launch("lstm2_update_forward");
}

template <int H>
int launch_update_backward(const Lstm2UpdBwd& b, hipStream_t s) {
    hipLaunchKernelGGL(lstm2_update_backward_kernel<H>, dim3(2u * (unsigned)b.n_wg), dim3(H / 16 * 64), 0, s, b);
    return check_launch("lstm2_update_backward");
}

}  // namespace
}  // namespace ppoaf

using namespace ppoaf;

// the layout the ctypes structure of _lib.py restates: K22's fields behind two 88-byte descriptors
#define PPOAF_LAYOUT(T, f, off) static_assert(offsetof(T, f) == off, #T "." #f)
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, actor, 0);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, critic, 88);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, params, 176);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, bucket_total, 208);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, step_counts, 232);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, norm_scratch_doubles, 256);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, beta1, 264);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, head_kind, 284);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, obs, 288);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, perm, 312);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, n_rows, 328);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, raw_actions, 344);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, values, 376);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, actor_hidden, 384);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, cursor, 416);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, B, 424);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, batch_stride, 432);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, normalize_values, 440);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, vn_mean, 448);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, adv_records, 480);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, normalize_adv, 488);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, surr_clip, 496);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, min_std, 512);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, loss_partials, 520);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, totals, 528);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, workspace, 536);
PPOAF_LAYOUT(ppoaf_lstm2_update_args_t, workspace_floats, 544);
static_assert(sizeof(ppoaf_lstm2_update_args_t) == 552, "ppoaf_lstm2_update_args_t");

extern "C" int ppoaf_lstm2_update_check(const ppoaf_lstm2_update_args_t* a, int32_t pointers) {
    return pointers ? check_update2_args(a) : check_update2_shapes(a);
}

extern "C" int ppoaf_lstm2_update_workspace_floats(const ppoaf_lstm2_update_args_t* a, int64_t* out) {
    if (int rc = check_update2_shapes(a)) return rc;
    PPOAF_REQUIRE(out != nullptr, "lstm2_update_workspace_floats: out is NULL");
    PPOAF_REQUIRE(a->bucket_total >= 1 && a->actor_size >= 1 && a->actor_size < a->bucket_total,
                  "lstm2_update_workspace_floats: bucket_total=%lld, actor_size=%lld", (long long)a->bucket_total, (long long)a->actor_size);
    Upd2Jobs J;
    PPOAF_REQUIRE(upd2_wgrad_jobs(a, J) > 0, "lstm2_update_workspace_floats: two weight-gradient jobs write one bucket element");
    out[0] = upd2_layout(*a).total;
    out[1] = norm2_doubles(a);
    out[2] = upd2_lds_bytes(a->actor.hidden);
    return PPOAF_OK;
}

extern "C" int ppoaf_lstm2_update_forward(const ppoaf_lstm2_update_args_t* a, ppoaf_stream_t stream) {
    Lstm2UpdDev v;
    if (int rc = make_dev2(a, v)) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (v.u.H) {
        case 32: return launch_update_forward<32>(v, s);
        case 64: return launch_update_forward<64>(v, s);
    }
    return launch_update_forward<128>(v, s);
}

extern "C" int ppoaf_lstm2_update_backward(const ppoaf_lstm2_update_args_t* a, ppoaf_stream_t stream) {
    Lstm2UpdDev v;
    if (int rc = make_dev2(a, v)) return rc;
    Lstm2UpdBwd b;
    b.net[0] = v.net[0]; b.net[1] = v.net[1]; b.n_wg = v.u.n_wg;
    hipStream_t s = (hipStream_t)stream;
    switch (v.u.H) {
        case 32: return launch_update_backward<32>(b, s);
        case 64: return launch_update_backward<64>(b, s);
    }
    return launch_update_backward<128>(b, s);
}

extern "C" int ppoaf_lstm2_update_wgrad(const ppoaf_lstm2_update_args_t* a, ppoaf_stream_t stream) {
    Lstm2UpdDev v;
    if (int rc = make_dev2(a, v)) return rc;
    Upd2Jobs J;
    const int nt = upd2_wgrad_jobs(a, J);
    PPOAF_REQUIRE(nt > 0, "lstm2_update_wgrad: two weight-gradient jobs write one bucket element");
    hipLaunchKernelGGL(lstm2_update_wgrad_kernel, dim3((unsigned)nt + 1u), dim3(256), 0, (hipStream_t)stream, J, v.u.grad_scale,
                       v.u.step_counts, v.u.norm_scratch);
    return check_launch("lstm2_update_wgrad");
}

extern "C" int ppoaf_lstm2_update_adam(const ppoaf_lstm2_update_args_t* a, ppoaf_stream_t stream) {
    Lstm2UpdDev v;
    if (int rc = make_dev2(a, v)) return rc;
    Upd2Jobs J;
    const int nt = upd2_wgrad_jobs(a, J);
    PPOAF_REQUIRE(nt > 0, "lstm2_update_adam: two weight-gradient jobs write one bucket element");
    return launch_update_adam(v.u, v.u.norm_scratch + 2, (unsigned)nt, (hipStream_t)stream, "lstm2_update_adam");
}
