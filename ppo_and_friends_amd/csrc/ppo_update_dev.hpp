// Shared by the fused PPO update kernels (ppo_update.hip: fwd_bwd and the separate reduce / Adam launches;
// ppo_update_split.hip, ppo_update_tail.hip: the split-wgrad chain): the device view of the C-ABI arguments, the job
// list of the split-wgrad launches and the distribution head + loss terms of one 16-row block.
#pragma once
#include "action_heads.hpp"
#include "running_stats_device.hpp"
#include "wgrad_tile.hpp"
#include <cstddef>
#include <cstring>

namespace ppoaf {

// Diagnostic build only (-DPPOAF_STAMPS): s_memtime per phase of workgroup (0, which), wave 0,
// into a buffer nothing else reads.  The shipped library executes no stamp.
// PPOAF_STAMP_W(k, w): the same clock read by lane 0 of wave w, into the buffer's second row (tools/phase_stamps.py:
// inside the head and the output backward, where the waves of a workgroup do different things).
#ifdef PPOAF_STAMPS
#ifndef PPOAF_STAMP_BLOCK
#define PPOAF_STAMP_BLOCK 0        /* 0..3: an actor workgroup, 4..7: a critic workgroup */
#endif
static __device__ unsigned long long g_ppo_update_stamps[2][16];
#define PPOAF_STAMP_AT(row, k, t0)                                                       \
    do {                                                                                 \
        if (blockIdx.x == PPOAF_STAMP_BLOCK && threadIdx.x == (t0)) {                    \
            unsigned long long t_;                                                       \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");    \
            g_ppo_update_stamps[row][k] = t_;                                            \
        }                                                                                \
    } while (0)
#define PPOAF_STAMP(k) PPOAF_STAMP_AT(0, k, 0)
#define PPOAF_STAMP_W(k, w) PPOAF_STAMP_AT(1, k, 64 * (w))
// The hidden forward layers of the row tile, every wave of the stamped workgroup (tools/phase_stamps.py): the clock is read
// into a register where the event is (PPOAF_HSTAMP, held in place by scheduling barriers) and stored behind the layer's
// barrier (PPOAF_HSTAMP_FLUSH) -- a store between the layer's own loads would queue with them.
static __device__ unsigned long long g_ppo_hidden_stamps[2][8][8];       // [layer][wave][event]
#define PPOAF_HSTAMP_DECL unsigned long long hstamp_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PPOAF_HSTAMP(k)                                                                  \
    do {                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                               \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hstamp_[k])::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                               \
    } while (0)
#define PPOAF_HSTAMP_FLUSH(layer)                                                        \
    do {                                                                                 \
        if (blockIdx.x == PPOAF_STAMP_BLOCK && (threadIdx.x & 63) == 0) {                \
            for (int k_ = 0; k_ < 8; ++k_) g_ppo_hidden_stamps[layer][threadIdx.x >> 6][k_] = hstamp_[k_]; \
        }                                                                                \
    } while (0)
#else
#define PPOAF_STAMP(k) do {} while (0)
#define PPOAF_STAMP_W(k, w) do {} while (0)
#define PPOAF_HSTAMP_DECL do {} while (0)
#define PPOAF_HSTAMP(k) do {} while (0)
#define PPOAF_HSTAMP_FLUSH(layer) do {} while (0)
#endif

// The instantiated (actor width, critic width) pairs of K6+K7 (policy_step.hip) and K12 (fwd_bwd, the wgrad launch, the
// fused tail): the ONE list.  Every dispatcher expands it into its `if` ladder and fwd_bwd_fits / the ladders' last line
// refuse what it does not name, so no launch can accept a pair that another one refuses.  A critic is never narrower than
// its actor here; a 512-wide network has a row-tile body of its own (ppo_update_rowtile_wide.hpp) and exists as a critic
// beside a 256-wide actor only.
// (three sub-lists: fwd_bwd's kernels are spread over ppo_update.hip, ppo_update_narrow.hip and ppo_update_wide.hip,
//  ppo_update_fwd_bwd.hpp)
// The WIDE sub-list is the one place where a launch refuses what the list names: its pair runs the three-launch form of the
// split-wgrad chain only (fwd_bwd -> ppoaf_ppo_update_wgrad -> ppoaf_ppo_update_adam(3)).  The fused tail
// (ppo_update_tail.hip) and the row-pair kernel have no instantiation for it -- the tail's ladder, PPOAF_WIDTH_PAIR_LADDER,
// runs over the pairs that have every launch form and answers "not instantiated" with the widths; pairs_run() needs a
// 256-wide critic -- and the host never asks for either (fused_update.py: tail_reason, pairs_reason).
#define PPOAF_WIDTH_PAIRS_IN_UPDATE(X) X(32, 32) X(64, 64) X(128, 128) X(256, 256) X(128, 256) X(64, 128)
#define PPOAF_WIDTH_PAIRS_IN_NARROW(X) X(64, 256) X(32, 256) X(32, 64)
#define PPOAF_WIDTH_PAIRS_WIDE(X) X(256, 512)
#define PPOAF_WIDTH_PAIRS_EVERY_FORM(X) PPOAF_WIDTH_PAIRS_IN_UPDATE(X) PPOAF_WIDTH_PAIRS_IN_NARROW(X)
#define PPOAF_WIDTH_PAIRS(X) PPOAF_WIDTH_PAIRS_EVERY_FORM(X) PPOAF_WIDTH_PAIRS_WIDE(X)
// one rung per pair: with PPOAF_WIDTH_PAIR_CALL_(A, C) defined as the expression that launches pair <A, C>,
// PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc) returns its value for the pair (ha, hc) and falls through for a pair not in the list
// (PPOAF_WIDTH_PAIR_LADDER_OF: over one of the sub-lists; PPOAF_WIDTH_PAIR_LADDER: the pairs with every launch form)
#define PPOAF_WIDTH_PAIR_RUNG_(A, C) if (ppoaf_ha_ == A && ppoaf_hc_ == C) return PPOAF_WIDTH_PAIR_CALL_(A, C);
#define PPOAF_WIDTH_PAIR_LADDER_OF(LIST, ha, hc) \
    { const int ppoaf_ha_ = (ha), ppoaf_hc_ = (hc); LIST(PPOAF_WIDTH_PAIR_RUNG_) }
#define PPOAF_WIDTH_PAIR_LADDER(ha, hc) PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_EVERY_FORM, ha, hc)
#define PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc) PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS, ha, hc)
inline bool width_pair_instantiated(const int ha, const int hc) {
#define PPOAF_WIDTH_PAIR_CALL_(A, C) true
    PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    return false;
}
inline bool width_pair_is_wide(const int ha, const int hc) {
#define PPOAF_WIDTH_PAIR_CALL_(A, C) true
    PPOAF_WIDTH_PAIR_LADDER_OF(PPOAF_WIDTH_PAIRS_WIDE, ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    return false;
}
// host: more than 8 actor outputs -- the wide heads' scope (fill_net has admitted 9 .. kWideOut at a 256-wide network): the head
// kinds that have them and, for the entry points with a critic, the width pair.  `what`: the entry point's name;
// critic_hidden: 0 where there is no critic (K19).
inline int check_wide_head(const char* what, const ppoaf_mlp_desc_t& actor, int head_kind, int critic_hidden) {
    if (actor.out_dim <= 8) return PPOAF_OK;
    PPOAF_REQUIRE(head_kind == PPOAF_HEAD_CATEGORICAL || head_kind == PPOAF_HEAD_GAUSSIAN,
                  "%s: actor out_dim=%d with head_kind=%d: the wide heads (out_dim 9 .. %d) are Categorical (0) and Gaussian (1); a "
                  "multi-categorical or Bernoulli head covers out_dim in [1,8]", what, actor.out_dim, head_kind, kWideOut);
    PPOAF_REQUIRE(critic_hidden == 0 || width_pair_is_wide(actor.hidden, critic_hidden),
                  "%s: actor out_dim=%d at hidden widths (actor %d, critic %d): the wide heads (out_dim 9 .. %d) exist for the wide "
                  "pair (actor 256, critic 512) only; this pair covers out_dim in [1,8]", what, actor.out_dim, actor.hidden,
                  critic_hidden, kWideOut);
    return PPOAF_OK;
}

// dynamic LDS of the wide critic's row-tile body (the carve of ppo_update_rowtile_wide.hpp): the row tables, biases, ONE
// output row of weights, the input rows, three activation-sized planes and the output / d output tiles.  No line slots:
// 124.7 KB at depth 7 and in_dim 64.
inline size_t rowtile_wide_lds_floats(const NetDev& n) {
    const size_t HS = n.H + 4, INP = 16 * ((n.in_dim + 15) / 16) + 4;
    return 208 + (size_t)(n.depth + 1) * n.H + (size_t)n.H + kRows * INP + 3 * kRows * HS + 2 * kRows * kMaxOut;
}
// dynamic LDS of the wide-head actor's row-tile body (the carve of ppo_update_rowtile_heads.hpp), without the line slots:
// rowtile_lds_floats' terms (ppo_update_rowtile.hpp) but for a floor under the input rows, whose region holds d loss / d out
// and the per-row d / d log_std, [16][24] each, once layer 0 has run -- more than the rows themselves below 33 inputs only.
constexpr int kHeadStride = kWideOut;                     // floats between the rows of the output tiles and the action words
constexpr int kHeadXFloats = 2 * kRows * kHeadStride;
inline size_t rowtile_heads_lds_floats(const NetDev& n) {
    const size_t HS = n.H + 4, INP = 16 * ((n.in_dim + 15) / 16) + 4;
    const size_t x = kRows * INP > (size_t)kHeadXFloats ? kRows * INP : (size_t)kHeadXFloats;
    return 208 + (size_t)(n.depth + 1) * n.H + 8 * (size_t)n.H + x + (size_t)n.depth * kRows * HS + 2 * kRows * HS +
           2 * kRows * kMaxOut;
}

// Per-mini-batch panels shared by the layered mode of the two-XCD persistent kernel and by the split-wgrad chain
// (fwd_bwd publishes them, the wgrad launch consumes them): workspace memory, 256-byte aligned pieces.
struct WsDev {
    float* hbuf[2];                       // [depth][Bp][H]   hidden activations of the mini-batch
    float* dbuf[2];                       // [depth][Bp][H]   dLoss / dz
    float* outpart[2];                    // [ceil(B/16)][seg] output-layer (+ log_std) gradient partials per row block
    float* xbuf[2];                       // [Bp][xld]        the mini-batch's gathered input rows, zero padded (layer-0 wgrad)
    int W;                                // workers per network (persistent kernel)
    // row stride of xbuf per network (split_xld): 64, or 128 for a wide pair's network with 64 < in_dim <= 128
    // (PPOAF_SPLIT_WIDE_INPUTS), 256 | 512 for one with in_dim <= 256 | 512 (PPOAF_SPLIT_WIDE_SHAPES).  Only the wide pair's kernels read it; every other kernel's stride is the constant 64.
    // (in the place of the persistent kernel's XCD numbers, which nothing read: the argument block keeps its layout)
    int xld[2];
    int Bp;                               // B rounded up to 64
};

struct UpdateDev {
    NetDev net[2];
    const float* params; float* grads; float* exp_avg; float* exp_avg_sq; float* slabs;
    long bucket_total;
    int64_t* step_counts; const float* lr; double* norm_scratch;
    float beta1, beta2, adam_eps, grad_scale, max_norm; int head_kind;
    const float* obs; const float* critic_obs; const void* raw_actions;
    const float* adv; const float* old_lp; const float* rtg; float* values;
    const int64_t* perm; const int32_t* row_map; long n_rows;
    int64_t* cursor; long B, batch_stride, mb_offset, cursor_advance;
    int normalize_values, n_ranks;
    float* vn_mean; float* vn_var; double* vn_count; const double* vn_records;
    const double* adv_records;
    int normalize_adv, use_huber, pregathered;
    float surr_clip, entropy_weight, kl_loss_weight, huber_delta, min_std;
    float* loss_partials; double* totals;
    int n_wg;
    int confine;         // args->xcd_half: 0 every XCD; 1 / 2: fwd_bwd's workgroups on XCDs 0-3 / 4-7 only (actor on two of them, critic on two)
    int split;           // 1: split-wgrad chain -- fwd_bwd publishes activation / dz panels (sp) instead of weight-gradient slabs
    WsDev sp;
    int n_slices; int slices[8];   // multi-categorical head: classes per action dimension (action_heads.hpp)
};

// offset of the output layer's segment (W_out, b_out, log_std) inside a network's bucket, and its length
inline long ws_seg_off(const NetDev& n) {
    const long szW0 = ((long)n.H * n.in_dim + 3) & ~3L;
    return n.depth == 0 ? 0 : szW0 + n.H + (long)(n.depth - 1) * ((long)n.H * n.H + n.H);
}
inline long ws_seg_len(const NetDev& n) { return n.size - ws_seg_off(n); }

// split-wgrad launch: one 4-wave workgroup per 16 x 32 piece of every layer's weight gradient (two MFMA tiles that share
// the dz operand and read whole 128-byte lines of the input panel; layer 0: ceil(in_dim / 32) pieces per 16 output rows)
// + one per network for the output layer's segment.  Jobs are dealt to workgroups in XCD-sized runs (workgroup b runs on
// XCD b % 8 and takes job (b % 8) * per_xcd + b / 8), so that a layer's panels are fetched by one or two XCDs instead of
// all eight; the bookkeeping workgroup comes last.
inline int split_wgrad_jobs(const NetDev& n) {
    const int t = n.H / 16, t2 = (t + 1) / 2, p0 = ((n.in_dim + 15) / 16 + 1) / 2;
    return (n.depth - 1) * t * t2 + t * p0 + 1;
}
inline int split_wgrad_per_xcd(const UpdateDev& u) { return (split_wgrad_jobs(u.net[0]) + split_wgrad_jobs(u.net[1]) + 7) / 8; }
inline int split_wgrad_blocks(const UpdateDev& u) { return 8 * split_wgrad_per_xcd(u); }      // some run no job (partials 0)

// args->row_pairs is a bit set (ppoaf_hip.h): the row pairs of 256-wide networks, the wide pair's 65 .. 128 inputs, the
// wide pair's in_dim <= 512 and B <= 1024 (which implies the second)
inline bool args_row_pairs(const ppoaf_ppo_update_args_t* a) { return (a->row_pairs & PPOAF_SPLIT_ROW_PAIRS) != 0; }
inline bool args_wide_shapes(const ppoaf_ppo_update_args_t* a) { return (a->row_pairs & PPOAF_SPLIT_WIDE_SHAPES) != 0; }
inline bool args_wide_inputs(const ppoaf_ppo_update_args_t* a) {
    return (a->row_pairs & (PPOAF_SPLIT_WIDE_INPUTS | PPOAF_SPLIT_WIDE_SHAPES)) != 0;
}

// row stride of a network's layer-0 panel, the smallest of 64, 128, 256, 512 that holds in_dim: the host admits in_dim > 64
// for a wide pair with PPOAF_SPLIT_WIDE_INPUTS (<= 128) or PPOAF_SPLIT_WIDE_SHAPES (<= 512) only (update_shapes,
// make_update_dev), so every other pair's panels are [Bp][64] as they always were
inline int split_xld(const NetDev& n) { return n.in_dim <= 64 ? 64 : n.in_dim <= 128 ? 128 : n.in_dim <= 256 ? 256 : 512; }

// workspace layout: per network hbuf, dbuf ([depth][Bp][H] each), outpart ([ceil(B/16)][seg]) and xbuf ([Bp][xld])
inline size_t ws_layout(const UpdateDev& u, WsDev* ws, char* base) {
    const long Bp = (u.B + 63) & ~63L;
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t o = off; off += (floats * 4 + 255) & ~(size_t)255; return o; };
    for (int w = 0; w < 2; ++w) {
        const NetDev& n = u.net[w];
        const size_t plane = (size_t)n.depth * Bp * n.H;
        const size_t oh = take(plane), od = take(plane), oo = take((size_t)((u.B + 15) / 16) * ws_seg_len(n));
        const size_t ox = take((size_t)Bp * split_xld(n));
        if (ws) {
            ws->hbuf[w] = reinterpret_cast<float*>(base + oh);
            ws->dbuf[w] = reinterpret_cast<float*>(base + od);
            ws->outpart[w] = reinterpret_cast<float*>(base + oo);
            ws->xbuf[w] = reinterpret_cast<float*>(base + ox);
            ws->xld[w] = split_xld(n);
        }
    }
    if (ws) ws->Bp = (int)Bp;
    return off;
}

// ---- row tiles of 256-wide networks on workgroup pairs (args->row_pairs; ppo_update_rowpair.hpp): the record region
constexpr int kPairHeaderBytes = 256;                 // word 0: error (a wait ran out of time)
constexpr int kPairRecBytes = 16 * 1024;              // a half panel (16 rows x 128 floats) as 1024 records of 16 bytes
constexpr int kPairMaxTiles = 32;                     // B <= 512 (split-wgrad chain)
constexpr long long kPairWaitTicks = 200000000LL;     // 2 s of wall_clock64 (100 MHz)

struct PairDev {
    unsigned char* base;                              // header, then per network [phase][tile][half] record blocks
    long net_off[2];                                  // byte offset of a network's blocks; 0: that network does not run in pairs
};

inline bool pair_eligible(const NetDev& n) { return n.H == 256 && n.depth >= 2 && n.depth <= 4; }
inline int pair_phases(const NetDev& n) { return 2 * n.depth - 3; }
// args->row_pairs takes effect (fwd_bwd's dispatch and ppoaf_ppo_update_row_pairs_error_offset both ask here): an eligible
// critic beside a narrower actor, whose tiles keep one workgroup each, or two eligible networks.  Other shapes (a 256-wide
// network of depth 1 or > 4, a 256-wide actor that is not eligible itself): one workgroup per tile.
inline bool pairs_run(const NetDev& a, const NetDev& c) {
    return width_pair_instantiated(a.H, c.H) && pair_eligible(c) && (a.H < 256 || pair_eligible(a));
}
// the region's place does not move with the mini-batch size (a tail mini-batch's panels are laid out differently, and
// nothing but records may ever be stored where records are polled): behind the panels of the FULL batch size
inline size_t pair_region_offset(const UpdateDev& u) {
    UpdateDev f = u;
    if (u.batch_stride > f.B) f.B = u.batch_stride;
    return ws_layout(f, nullptr, nullptr);
}
inline size_t pair_region_layout(const UpdateDev& u, PairDev* p, char* region) {
    size_t off = kPairHeaderBytes;
    for (int w = 0; w < 2; ++w) {
        const bool on = pair_eligible(u.net[w]);
        if (p) p->net_off[w] = on ? (long)off : 0;
        if (on) off += (size_t)pair_phases(u.net[w]) * kPairMaxTiles * 2 * kPairRecBytes;
    }
    if (p) p->base = reinterpret_cast<unsigned char*>(region);
    return off;
}

constexpr int kWgradThreads = 256;

// One job of a network's layer-major job list (split_wgrad_jobs): a 16 x 32 piece of layer l's dW -- output tile ot, input
// tiles itile and itile + 1 (the second may not exist: odd tile counts) -- or, behind those, the output layer's segment.
// Offsets are floats inside the network's part of the bucket.
struct SplitJob {
    int l, ot, itile;
    bool two;                                             // uniform per workgroup
    long ldw;                                             // row stride of W_l
    long off_w, off_b;                                    // W_l, b_l
};
template <int H>
__device__ __forceinline__ long split_off_w(const NetDev& nd, const int l) {
    const long szW0 = ((long)H * nd.in_dim + 3) & ~3L;
    return l == 0 ? 0 : szW0 + H + (long)(l - 1) * ((long)H * H + H);
}
// false: `job` is the network's output-segment job (which starts at split_off_w<H>(nd, nd.depth))
template <int H>
__device__ __forceinline__ bool split_job_decode(const UpdateDev& u, const int which, const int job, SplitJob& sj) {
    const auto& nd = u.net[which];
    const int in_dim = nd.in_dim, depth = nd.depth;
    constexpr int t = H / 16, t2 = (t + 1) / 2;
    const int n_it0 = (in_dim + 15) / 16, p0 = (n_it0 + 1) / 2;
    const int n_hidden = (depth - 1) * t * t2, n_l0 = t * p0;
    if (job >= n_hidden + n_l0) return false;
    int n_it;
    if (job < n_hidden) { sj.l = 1 + job / (t * t2); const int jj = job % (t * t2); sj.ot = jj / t2; sj.itile = 2 * (jj % t2); n_it = t; }
    else { sj.l = 0; const int jj = job - n_hidden; sj.ot = jj / p0; sj.itile = 2 * (jj % p0); n_it = n_it0; }
    const int l = sj.l;
    sj.two = sj.itile + 1 < n_it;
    sj.ldw = l >= 1 ? H : in_dim;
    sj.off_w = split_off_w<H>(nd, l);
    sj.off_b = l == 0 ? (((long)H * in_dim + 3) & ~3L)
                      : sj.off_w + (l < depth ? (long)H * H : (((long)nd.out_dim * H + 3) & ~3L));
    return true;
}
// layer l's dz panel and input panel (the mini-batch's gathered input rows for layer 0) as buffer resources
template <int H> __device__ __forceinline__ __amdgpu_buffer_rsrc_t split_panel_d(const UpdateDev& u, const int which, const int l) {
    return wgrad_rsrc(u.sp.dbuf[which] + (long)l * ((long)u.sp.Bp * H));
}
template <int H> __device__ __forceinline__ __amdgpu_buffer_rsrc_t split_panel_x(const UpdateDev& u, const int which, const int l) {
    return wgrad_rsrc(l >= 1 ? u.sp.hbuf[which] + (long)(l - 1) * ((long)u.sp.Bp * H) : u.sp.xbuf[which]);
}
// Element idx of the output layer's segment (+ log_std): fwd_bwd's row-block partials added in block order, 8 in flight
__device__ __forceinline__ float split_out_fold(const float* outpart, const int n_hb, const long seg_len, const long idx) {
    float acc = 0.f;
    for (int g0 = 0; g0 < n_hb; g0 += 8) {
        float pv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) pv[k] = outpart[(long)(g0 + k < n_hb ? g0 + k : 0) * seg_len + idx];
#pragma unroll
        for (int k = 0; k < 8; ++k) if (g0 + k < n_hb) acc += pv[k];
    }
    return acc;
}

// per-mini-batch bookkeeping of the split-wgrad chain, by ONE wave (threads 0..63 of a workgroup): loss partials -> totals
__device__ __forceinline__ void ppo_update_bookkeeping_totals(const UpdateDev& u) {
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
    }
}
// ... and the step counters + Adam bias corrections of the step being taken
__device__ __forceinline__ void ppo_update_bookkeeping_steps(const UpdateDev& u) {
    const int lane = threadIdx.x;
    if (lane < 2) {                                       // one lane per network: step counter + bias corrections
        const int w = lane;
        const int64_t t = u.step_counts[w] + 1;
        u.step_counts[w] = t;
        u.norm_scratch[2 + 2 * w] = 1.0 - pow((double)u.beta1, (double)t);
        u.norm_scratch[3 + 2 * w] = sqrt(1.0 - pow((double)u.beta2, (double)t));
    }
}

__device__ __forceinline__ void ppo_update_bookkeeping_split(const UpdateDev& u) {
    if (threadIdx.x >= 64) return;
    ppo_update_bookkeeping_totals(u);
    ppo_update_bookkeeping_steps(u);
}

// host: validate ppoaf_ppo_update_args_t and fill the device view (ppo_update.hip)
int make_update_dev(const ppoaf_ppo_update_args_t* a, UpdateDev& u);

// host: a private copy of the caller's args.  The slice table appended to the struct is read only for the head kind that
// has one, so a caller built against a header without it is never read past the end of its struct.
inline ppoaf_ppo_update_args_t copy_update_args(const ppoaf_ppo_update_args_t* args) {
    ppoaf_ppo_update_args_t a;
    std::memset(&a, 0, sizeof(a));
    std::memcpy(&a, args, offsetof(ppoaf_ppo_update_args_t, n_action_slices));
    if (args->head_kind == PPOAF_HEAD_MULTI_CATEGORICAL) {
        a.n_action_slices = args->n_action_slices;
        std::memcpy(a.action_slices, args->action_slices, sizeof(a.action_slices));
    }
    return a;
}

__device__ __forceinline__ unsigned hw_xcc_id() {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xfu;
}

// K6 + K3 for the 16 rows of block g of network `which` (0 actor, 1 critic), run by ONE wave (lanes 0..15 hold a
// row each; the categorical head uses 4 lanes per row; the multi-categorical and Bernoulli heads take their log-prob
// from the functions K6 uses, action_heads.hpp): distribution head on the output-layer values sOut[16][16],
// PPO / value loss terms (ppo.py:2325-2438), d loss / d out -> sDOut[16][16] (and, Gaussian head, per-row
// d / d log_std parked in sOut[.][8..]), the block's loss partials -> u.loss_partials, critic values written back.
//   sRow16[16] dataset row of each block row (-1: dead), sRowF[3][16] adv / old log-prob / rewards-to-go,
//   sMisc[4] adv mean / std, value-normaliser mean / var, sActF[16][8] raw actions, log_std_p the actor's log_std.
// In three parts, so that a caller can take everything the backward pass does not wait for off its path:
//   ppo_head_rows    the row part: everything up to sDOut (and sOut[.][8..]).  Touches no global memory but the Gaussian
//                    head's log_std.  It leaves each row's loss terms (part[0, 2, 3, 4, 7]; dead rows: zeros) in the row's
//                    8 words of sActF, which is dead once the row's actions have been read.
//   ppo_head_values  the critic's u.values[row] = v (ppo.py:2340), from sOut alone.
//   ppo_head_block   the block part: the parked terms, read in row order, -> the same eight 16-lane sums -> u.loss_partials.
// The last two may run on any wave, any time after a barrier behind the row part, while sRow / sOut / sActF are intact.
// HEAD: the actor's head kind as a compile-time constant (ppo_update_lean.hip: the arms of the other heads leave the text),
// or -1: read from u.head_kind where each arm asks, as every other caller does.
template <int HEAD, typename U>
__device__ __forceinline__ int head_kind_as(const U& u) {
    if constexpr (HEAD >= 0) return HEAD;
    else return u.head_kind;
}
template <int HEAD = -1, typename U>
__device__ __forceinline__ void ppo_head_rows(const U& u, const int which, const int out_dim,
                                              const float* __restrict__ log_std_p, const int* sRow,
                                              const float* sRowF, const float* sMisc, float* sActF, float* sOut,
                                              float* sDOut, const int lane, const long B) {
    const int s = lane;                       // lanes 0..15 hold one row each
    const int row = s < kRows ? sRow[s] : -1;
    const bool live = row >= 0;
    const float inv_B = 1.0f / (float)B;
    float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (which == 0) {
        float logp = 0.f, ent = 0.f;
        float av = 0.f, lpo = 0.f;
        if (live) {
            av = sRowF[s]; lpo = sRowF[16 + s];
            if (u.normalize_adv) av = (av - sMisc[0]) / (sMisc[1] + 1e-8f);
        }
        if (head_kind_as<HEAD>(u) == PPOAF_HEAD_CATEGORICAL) {
            // lane-parallel: 4 lanes per row, lane (s4, q) owns classes q and q + 4; the class
            // reductions are two xor-shuffles inside the 4-lane group, so the transcendental chain
            // is 2 values long instead of 8.  Row results are handed to lane s4 at the end.
            const int s4 = lane >> 2, q = lane & 3;
            const bool live4 = sRow[s4] >= 0;
            float av4 = 0.f, lpo4 = 0.f;
            if (live4) {
                av4 = sRowF[s4]; lpo4 = sRowF[16 + s4];
                if (u.normalize_adv) av4 = (av4 - sMisc[0]) / (sMisc[1] + 1e-8f);
            }
            auto rsum = [](float v) { return group4_sum(v); };       // xor 1, xor 2 as DPP quad permutes (mlp_device.hpp)
            auto rmax = [](float v) { return group4_max(v); };
            const int k0 = q, k1 = q + 4;
            const bool v0 = k0 < out_dim, v1 = k1 < out_dim;
            const float z0 = v0 ? sOut[s4 * kMaxOut + k0] : -INFINITY, z1 = v1 ? sOut[s4 * kMaxOut + k1] : -INFINITY;
            const float m = rmax(fmaxf(z0, z1));
            float p0 = v0 ? expf(z0 - m) : 0.f, p1 = v1 ? expf(z1 - m) : 0.f;
            const float inv = 1.0f / rsum(p0 + p1);
            p0 *= inv; p1 *= inv;
            const float s2 = rsum(p0 + p1);
            int a = reinterpret_cast<const int*>(sActF)[s4 * 8];
            a = a < 0 ? 0 : (a >= out_dim ? out_dim - 1 : a);
            const float n0 = p0 / s2, n1 = p1 / s2;                          // Categorical's renormalisation
            const float l0 = v0 ? logf(clamp_prob_u(n0)) : 0.f, l1 = v1 ? logf(clamp_prob_u(n1)) : 0.f;
            const float ent4 = -rsum((v0 ? n0 * l0 : 0.f) + (v1 ? n1 * l1 : 0.f));
            const float logp4 = rsum((k0 == a ? l0 : 0.f) + (k1 == a ? l1 : 0.f));
            const float ratio = expf(logp4 - lpo4);
            const float bad4 = (isnan(ratio) || isinf(ratio)) ? 1.f : 0.f;
            const float lo = 1.0f - u.surr_clip, hi = 1.0f + u.surr_clip;
            const float surr1 = ratio * av4, surr2 = fminf(fmaxf(ratio, lo), hi) * av4;
            float glp;
            if (surr1 <= surr2) glp = -av4 * ratio;
            else glp = (ratio >= lo && ratio <= hi) ? -av4 * ratio : 0.f;
            glp *= inv_B;
            const float gH = (u.entropy_weight != 0.0f) ? -u.entropy_weight * inv_B : 0.f;
            // chain: z -softmax-> p -(/sum)-> n -clamp,log-> l
            auto gk_of = [&](bool valid, int k, float nk, float lg) {
                if (!valid) return 0.f;
                const float ck = clamp_prob_u(nk);
                const float in_range = (nk >= FLT_EPSILON && nk <= 1.0f - FLT_EPSILON) ? 1.f : 0.f;
                float gk = gH * (-lg - nk * in_range / ck);
                if (k == a) gk += glp * in_range / ck;
                return gk;
            };
            float g0 = gk_of(v0, k0, n0, l0), g1 = gk_of(v1, k1, n1, l1);
            const float dot = rsum(g0 * n0 + g1 * n1);
            g0 = (g0 - dot) / s2; g1 = (g1 - dot) / s2;
            const float dot2 = rsum(g0 * p0 + g1 * p1);
            if (live4) {
                if (k0 < 8) sDOut[s4 * kMaxOut + k0] = p0 * (g0 - dot2);
                sDOut[s4 * kMaxOut + k1] = p1 * (g1 - dot2);
            } else {
                sDOut[s4 * kMaxOut + k0] = 0.f; sDOut[s4 * kMaxOut + k1] = 0.f;
                if (q == 0) for (int k2 = 8; k2 < kMaxOut; ++k2) sDOut[s4 * kMaxOut + k2] = 0.f;
            }
            // row results: lane (s4, 0) holds them; it parks them below
            if (live4) { part[0] = -fminf(surr1, surr2); part[3] = ent4; part[4] = lpo4 - logp4; part[7] = bad4; }
        } else if (head_kind_as<HEAD>(u) >= PPOAF_HEAD_MULTI_CATEGORICAL) {
            // MultiDiscrete / MultiBinary (action_heads.hpp): one lane per row
            if (live) {
                float z[8], dz[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) z[k] = k < out_dim ? sOut[s * kMaxOut + k] : 0.f;
                const bool mcat = head_kind_as<HEAD>(u) == PPOAF_HEAD_MULTI_CATEGORICAL;
                const float* x = sActF + s * 8;
                float p[8], sm[8];
                unsigned first = 0u, pick = 0u;
                if (mcat) {
                    first = mcat_starts(u.n_slices, u.slices);
                    mcat_probs(z, first, out_dim, p, sm);
                    pick = mcat_pick(reinterpret_cast<const int*>(x), u.n_slices, u.slices);
                    logp = mcat_logp(p, sm, pick);
                } else {
                    logp = bern_logp(z, x, out_dim);
                }
                const float ratio = expf(logp - lpo);
                if (isnan(ratio) || isinf(ratio)) part[7] = 1.f;
                const float lo = 1.0f - u.surr_clip, hi = 1.0f + u.surr_clip;
                const float surr1 = ratio * av, surr2 = fminf(fmaxf(ratio, lo), hi) * av;
                float glp;
                if (surr1 <= surr2) glp = -av * ratio;
                else glp = (ratio >= lo && ratio <= hi) ? -av * ratio : 0.f;
                glp *= inv_B;
                const float gH = (u.entropy_weight != 0.0f) ? -u.entropy_weight * inv_B : 0.f;
                ent = mcat ? mcat_entropy_grad(p, sm, first, pick, out_dim, glp, gH, dz)
                           : bern_entropy_grad(z, x, out_dim, glp, gH, dz);
                part[0] = -fminf(surr1, surr2);
                part[3] = ent;
                part[4] = lpo - logp;
#pragma unroll
                for (int k = 0; k < 8; ++k) sDOut[s * kMaxOut + k] = dz[k];
            } else if (s < kRows) {
                for (int k = 0; k < kMaxOut; ++k) sDOut[s * kMaxOut + k] = 0.f;
            }
        } else if (live) {
            // tanh-Gaussian (distributions.py:441-694)
            const float* log_std = log_std_p;
            const float* x = sActF + s * 8;
            float lp = 0.f, slog = 0.f;
            ent = 0.f;
            for (int d = 0; d < out_dim; ++d) {
                const float sd = fmaxf(softplus_u(log_std[d]), u.min_std);
                const float mu = sOut[s * kMaxOut + d];
                const float zz = x[d] - mu;
                const float l0 = -logf(sd) - 0.91893853320467274178f;
                float l = -(zz * zz) / (2.0f * sd * sd) + l0;
                l = fminf(fmaxf(l, -100.f), 100.f);
                lp += l;
                const float th = tanhf(x[d]);
                slog += logf(fmaxf(1.0f - th * th, 1e-6f));
                // entropy := -log_prob of the distribution's MEAN (ppo_policy.py:950, distributions.py:672-694)
                const float thm = tanhf(mu);
                ent += logf(fmaxf(1.0f - thm * thm, 1e-6f)) - fminf(fmaxf(l0, -100.f), 100.f);
            }
            logp = lp - slog;
            const float ratio = expf(logp - lpo);
            if (isnan(ratio) || isinf(ratio)) part[7] = 1.f;
            const float lo = 1.0f - u.surr_clip, hi = 1.0f + u.surr_clip;
            const float surr1 = ratio * av, surr2 = fminf(fmaxf(ratio, lo), hi) * av;
            part[0] = -fminf(surr1, surr2);
            part[3] = ent;
            part[4] = lpo - logp;
            float glp;
            if (surr1 <= surr2) glp = -av * ratio;
            else glp = (ratio >= lo && ratio <= hi) ? -av * ratio : 0.f;
            glp *= inv_B;
            const float gH = (u.entropy_weight != 0.0f) ? -u.entropy_weight * inv_B : 0.f;
            for (int d = 0; d < out_dim; ++d) {
                const float ls = log_std[d];
                const float sp = softplus_u(ls), sd = fmaxf(sp, u.min_std);
                const float mu = sOut[s * kMaxOut + d];
                const float zz = x[d] - mu;
                const float l0 = -logf(sd) - 0.91893853320467274178f;
                const float l = -(zz * zz) / (2.0f * sd * sd) + l0;
                const float pass = (l >= -100.f && l <= 100.f) ? 1.f : 0.f;
                const float pass0 = (l0 >= -100.f && l0 <= 100.f) ? 1.f : 0.f;
                const float thm = tanhf(mu);
                const float pass_t = (1.0f - thm * thm >= 1e-6f) ? 1.f : 0.f;
                sDOut[s * kMaxOut + d] = glp * pass * zz / (sd * sd) - gH * pass_t * 2.0f * thm;
                if (d == 0) for (int k2 = out_dim; k2 < 8; ++k2) sDOut[s * kMaxOut + k2] = 0.f;
                const float dmax = sp > u.min_std ? 1.f : (sp == u.min_std ? 0.5f : 0.f);
                const float dsp = ls > 20.f ? 1.f : 1.0f / (1.0f + expf(-ls));
                // per-row d logp / d log_std, parked in sOut's upper half for the reduction below
                sOut[s * kMaxOut + 8 + d] = (glp * pass * (zz * zz / (sd * sd * sd) - 1.0f / sd) + gH * pass0 / sd) * dmax * dsp;
            }
        } else if (s < kRows) {
            for (int k = 0; k < kMaxOut; ++k) sDOut[s * kMaxOut + k] = 0.f;
            if (head_kind_as<HEAD>(u) == PPOAF_HEAD_GAUSSIAN)
                for (int d = 0; d < 8; ++d) sOut[s * kMaxOut + 8 + d] = 0.f;
        }
    } else {
        if (live) {
            const float v = sOut[s * kMaxOut];
            float rt = sRowF[32 + s];
            if (u.normalize_values) rt = (rt - sMisc[2]) / sqrtf(sMisc[3] + 1e-8f);
            const float diff = v - rt;
            float l, dl;
            if (u.use_huber) {
                const float ad = fabsf(diff);
                if (ad < u.huber_delta) { l = 0.5f * diff * diff; dl = diff; }
                else { l = u.huber_delta * (ad - 0.5f * u.huber_delta); dl = diff > 0.f ? u.huber_delta : -u.huber_delta; }
            } else { l = diff * diff; dl = 2.0f * diff; }
            part[2] = l;
            sDOut[s * kMaxOut] = dl * inv_B;
            for (int k2 = 1; k2 < 8; ++k2) sDOut[s * kMaxOut + k2] = 0.f;
        } else if (s < kRows) {
            for (int k2 = 0; k2 < 8; ++k2) sDOut[s * kMaxOut + k2] = 0.f;
        }
    }
    // park the row's terms where its actions were.  (The actions were read above through pointers of another type: the
    // compiler may not take these stores ahead of those reads.)
    asm volatile("" ::: "memory");
    const bool cat = which == 0 && head_kind_as<HEAD>(u) == PPOAF_HEAD_CATEGORICAL;
    const int prow = cat ? (lane >> 2) : s;
    if (cat ? (lane & 3) == 0 : s < kRows) {
        float* pk = sActF + prow * 8;
        pk[0] = part[0]; pk[2] = part[2]; pk[3] = part[3]; pk[4] = part[4]; pk[7] = part[7];
    }
}

template <typename U>
__device__ __forceinline__ void ppo_head_values(const U& u, const int* sRow, const float* sOut, const int lane) {
    if (lane < kRows) {
        const int row = sRow[lane];
        if (row >= 0) u.values[row] = sOut[lane * kMaxOut];      // ppo.py:2340
    }
}

template <typename U>
__device__ __forceinline__ void ppo_head_block(const U& u, const int which, const int g, const float* sMisc,
                                               const float* sActF, const int lane) {
    float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane < kRows) {
        const float* pk = sActF + lane * 8;
        part[0] = pk[0]; part[2] = pk[2]; part[3] = pk[3]; part[4] = pk[4]; part[7] = pk[7];
    }
    // per-workgroup partial sums (lanes >= 16 contribute zeros)
#pragma unroll
    for (int k = 0; k < 8; ++k) part[k] = group16_sum(part[k]);
    if (lane == 0) {
        if (which == 0 && g == 0) { part[5] = sMisc[0]; part[6] = sMisc[1]; }
        float* lp = u.loss_partials + ((long)which * u.n_wg + g) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) lp[k] = part[k];
    }
}

// the three parts back to back on one wave (the pair body, ppo_update_rowpair.hpp; K22, lstm_update.hip)
template <typename U>
__device__ __forceinline__ void ppo_head_loss(const U& u, const int which, const int g, const int out_dim,
                                              const float* __restrict__ log_std_p, const int* sRow,
                                              const float* sRowF, const float* sMisc, float* sActF, float* sOut,
                                              float* sDOut, const int lane, const long B) {
    ppo_head_rows(u, which, out_dim, log_std_p, sRow, sRowF, sMisc, sActF, sOut, sDOut, lane, B);
    if (which != 0) ppo_head_values(u, sRow, sOut, lane);
    ppo_head_block(u, which, g, sMisc, sActF, lane);
}

}  // namespace ppoaf
