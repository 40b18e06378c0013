// The row-tiled forward + backward of one 16-row block of one network (K12's fwd_bwd kernel body; ppo_update.hip).
#pragma once
#include "ppo_update_dev.hpp"

namespace ppoaf {

extern __shared__ __attribute__((aligned(16))) unsigned char ppo_update_smem[];


// SPLIT = true (split-wgrad chain): the body keeps forward, losses and dgrad, but computes NO weight gradient of a hidden
// layer.  It publishes what a complete-K wgrad launch needs instead -- its 16 rows of the input x, of every hidden
// activation h_l and of every dLoss/dz_l (u.sp: hbuf / dbuf / xbuf planes, 16 KB per layer per workgroup at H = 128
// against a 135 KB slab) -- and the output layer's partials go to u.sp.outpart (folded in block order by that launch).

// (A forward weight set of one output tile is requested as whole lines, load_fwd_lines_buf, and turned into fragment order
//  through the wave's LDS slots when consumed, mfma_rows_x_lines: one CU's L1 delivers the fragment pattern itself at a
//  third of that rate.)

// The kernel arguments the prologue of a row-tile workgroup needs, asked for in ONE batch at the kernel's entry.  Left to
// itself the compiler fetches the 1176-byte argument block field group by field group as the code reaches each use, every
// group with a wait of its own and nothing else in flight (nine of them ahead of the first vector load, the cursor's the
// fourth).  An empty asm that takes the fields as scalar inputs makes all of them due at one point: their loads go out
// together, one wait covers them, and the uses below find the values in registers (kernel-argument loads are invariant:
// the same field is not fetched twice as long as it stays in a register or in a lane of the spill register).  The cursor
// and the fields both flavours of the body read first make the second trip: 2 scalar waits ahead of the first vector
// load, of 9.  Both networks' descriptors: a workgroup's network is chosen behind this point.
__device__ __forceinline__ int rowtile_request_args(const UpdateDev& u, int b) {
    // (`b`, the workgroup's number, goes through the statement: everything below depends on it, so the statement stays
    //  where it is without being volatile -- a volatile asm counts as a store to anywhere, and the cursor's load behind it
    //  would no longer be a scalar load)
    const NetDev& a = u.net[0];
    const NetDev& c = u.net[1];
    // (fields the prologue has no use for are on the list where they lie between ones it needs: adjacent fields are
    //  fetched by one wide load, and a register of that load that nobody reads is handed to the next load at once --
    //  which then has to wait for the wide one first)
    asm("" : "+s"(b)
        : "s"(a.in_dim), "s"(a.H), "s"(a.depth), "s"(a.out_dim), "s"(a.act), "s"((&a.act)[1]), "s"(a.offset), "s"(a.size), "s"(a.log_std_off),
          "s"(c.in_dim), "s"(c.H), "s"(c.depth), "s"(c.out_dim), "s"(c.act), "s"((&c.act)[1]), "s"(c.offset), "s"(c.size), "s"(c.log_std_off),
          "s"(u.params), "s"(u.norm_scratch), "s"(u.head_kind),
          "s"(u.obs), "s"(u.critic_obs), "s"(u.raw_actions), "s"(u.adv), "s"(u.old_lp), "s"(u.rtg), "s"(u.values), "s"(u.perm),
          "s"(u.row_map), "s"(u.n_rows), "s"(u.cursor), "s"(u.B), "s"(u.batch_stride), "s"(u.mb_offset), "s"(u.cursor_advance),
          "s"(u.normalize_values), "s"(u.n_ranks), "s"(u.vn_mean), "s"(u.vn_var), "s"(u.vn_count), "s"(u.vn_records),
          "s"(u.adv_records), "s"(u.normalize_adv), "s"(u.use_huber), "s"(u.pregathered), "s"(u.surr_clip),
          "s"(u.n_wg), "s"(u.confine));
    // second trip: the cursor itself, and with it what both flavours of the body read first behind their dispatch (the
    // compiler hoists those loads to the dispatch and parks them in lanes of a vector register at once -- two more waits)
    const long cur = u.cursor[0];
    asm("" : "+s"(b)
        : "s"(cur), "s"(u.entropy_weight), "s"(u.kl_loss_weight), "s"(u.huber_delta), "s"(u.min_std), "s"(u.loss_partials),
          "s"(u.sp.hbuf[0]), "s"(u.sp.hbuf[1]), "s"(u.sp.dbuf[0]), "s"(u.sp.dbuf[1]), "s"(u.sp.outpart[0]), "s"(u.sp.outpart[1]),
          "s"(u.sp.xbuf[0]), "s"(u.sp.xbuf[1]), "s"(u.sp.W), "s"(u.sp.xld[0]), "s"(u.sp.xld[1]), "s"(u.sp.Bp), "s"(u.n_slices),
          "s"(u.slices[0]), "s"(u.slices[1]), "s"(u.slices[2]), "s"(u.slices[3]), "s"(u.slices[4]), "s"(u.slices[5]),
          "s"(u.slices[6]), "s"(u.slices[7]));
    return b;
}

// CP adjacent floats of LDS <-> registers; 16-byte accesses where CP allows (the callers' addresses are multiples of CP floats)
template <int CP> __device__ __forceinline__ void lds_read_adjacent(const float* p, float (&v)[CP]) {
    if constexpr (CP % 4 == 0) {
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * q);
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < CP; ++q) v[q] = p[q];
    }
}
template <int CP> __device__ __forceinline__ void lds_write_adjacent(float* p, const float (&v)[CP]) {
    if constexpr (CP % 4 == 0) {
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) *reinterpret_cast<float4*>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
        for (int q = 0; q < CP; ++q) p[q] = v[q];
    }
}

// TABLES is the flavour the epoch driver of fused_update.py runs at three hidden layers: the deep prefetch below (one
// output tile per wave) over per-epoch tables in shuffled order that hold row numbers (u.pregathered, no u.row_map).  It is
// a compile-time flavour, chosen by ppo_update_fwd_bwd_body from the arguments.  As run-time conditions of one body, "are
// the hidden sets requested" and "do a row's scalars follow the sets as dependent loads" left the compiler several
// histories to reconcile at every later wait of the prologue, and its safe answer to that is vmcnt(0): each of those waits
// then waited for the sets as well.  Every other case runs the body as it was (TABLES = false: both decided at run time).
// XLD (the wide pair's kernel only, ppo_update_fwd_bwd.hpp): the SPLIT publish of the input rows takes the panel's row stride
// from u.sp.xld[which] (64 | 128: PPOAF_SPLIT_WIDE_INPUTS; 256 | 512: PPOAF_SPLIT_WIDE_SHAPES).  Every other kernel keeps the constant and the loop written for it.
// ACT / HEAD (ppo_update_lean.hip): the network's activation code and the actor's head kind as compile-time constants -- what a
// training run never changes is then not decided in every workgroup of every launch, and the other activations' and heads'
// arms leave the text.  -1 (every other caller): read from the arguments.
template <int HT, bool SPLIT, bool TABLES, bool XLD = false, int ACT = -1, int HEAD = -1>
__device__ __forceinline__ void ppo_update_fwd_bwd_body_as(const UpdateDev& u, const int which, const int g) {
    constexpr int H = 16 * HT, HS = H + 4;                 // which: 0 actor, 1 critic; g: 16-row block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto& nd = u.net[which];
    const int in_dim = nd.in_dim, depth = nd.depth, out_dim = nd.out_dim, act = ACT >= 0 ? ACT : nd.act;
    const int NT0 = (in_dim + 15) >> 4;                    // 16-column tiles of the input
    const int INP = 16 * NT0 + 4;
    const float* P = u.params + nd.offset;
    const long B = u.B;
    const long mb = u.cursor[0] + u.mb_offset;
    const long base = mb * u.batch_stride;
    // Layer offsets inside the bucket, by arithmetic: indexing a table in the kernel arguments with a
    // loop variable compiles to a vector load of kernarg memory plus a full vmcnt drain (~6k cycles).
    const long szW0 = ((long)H * in_dim + 3) & ~3L;
    auto offW = [&](int l) -> long { return l == 0 ? 0 : szW0 + H + (long)(l - 1) * (H * H + H); };
    auto offB = [&](int l) -> long {
        return l == 0 ? szW0 : offW(l) + (l < depth ? (long)H * H : (((long)out_dim * H + 3) & ~3L));
    };
    // where this block's gradient partials go: its slab of the whole bucket, or (SPLIT: only the output layer's segment is
    // produced here) its row of the output-layer partials, addressed with the same bucket offsets
    float* slab = SPLIT ? u.sp.outpart[which] + (long)g * (nd.size - offW(depth)) - offW(depth)
                        : u.slabs + (long)g * u.bucket_total + nd.offset;
    // 16 rows x H floats of LDS (row stride HS) -> rows [16 g, +16) of a [Bp][H] panel: one float4 per thread at H = 128.
    // In two halves: the LDS read where the rows are complete, the stores behind the MFMAs of the layer that consumes the
    // same rows.  Nothing reads the panel before the next launch, and a wave issues in order: a store ahead of the layer
    // would put the LDS round trip of its data in front of the layer's first MFMA.
    // (256-wide tiles keep the store at the read: their register file is full, two more float4 across the MFMAs spill)
    constexpr int kPub = (kRows * (H / 4) + kThreadsU - 1) / kThreadsU;
    constexpr bool kPubLate = HT <= kNW;
    float4 pub[kPub];
    auto publish_read = [&](const float* src) {
#pragma unroll
        for (int q = 0; q < kPub; ++q) {
            const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
            if (i < kRows * (H / 4)) pub[q] = *reinterpret_cast<const float4*>(src + r * HS + 4 * c4);
        }
    };
    auto publish_store = [&](float* panel) {
        float* dst = panel + (long)g * kRows * H;
#pragma unroll
        for (int q = 0; q < kPub; ++q) {
            const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
            if (i < kRows * (H / 4)) *reinterpret_cast<float4*>(dst + (long)r * H + 4 * c4) = pub[q];
        }
    };
    // ahead of a layer's MFMAs / behind them (the scheduling barrier keeps the compiler from taking the stores back up)
    auto publish_begin = [&](const float* src, float* panel) {
        publish_read(src);
        if constexpr (!kPubLate) publish_store(panel);
    };
    auto publish_end = [&](float* panel) {
        if constexpr (kPubLate) { __builtin_amdgcn_sched_barrier(0); publish_store(panel); }
    };
    const long sp_plane = SPLIT ? (long)u.sp.Bp * H : 0;

    PPOAF_STAMP(0);
    PPOAF_HSTAMP_DECL;
    // ---- LDS carve (all offsets multiples of 16 B)
    float* smem = reinterpret_cast<float*>(ppo_update_smem);
    int* sRow = reinterpret_cast<int*>(smem);                 // [16]
    float* sMisc = smem + 16;                                 // [16]: adv mean/std, vn mean/var
    float* sRowF = smem + 32;                                 // [3][16]: adv, old log-prob, rewards-to-go
    float* sActF = smem + 80;                                 // [16][8] raw actions (float or int bits)
    float* sBias = smem + 208;                                // [(depth+1), H]
    float* sWout = sBias + (depth + 1) * H;                   // [8, H]
    float* sX = sWout + 8 * H;                                // [16, INP], zero padded
    float* sH = sX + kRows * INP;                             // depth x [16, HS]
    float* sD0 = sH + (long)depth * kRows * HS;               // [16, HS]
    float* sD1 = sD0 + kRows * HS;                            // [16, HS]
    float* sOut = sD1 + kRows * HS;                           // [16, 16]
    float* sDOut = sOut + kRows * kMaxOut;                    // [16, 16]
    float* sScr = sDOut + kRows * kMaxOut + wave * 2 * kLineSlot;   // this wave's two line slots

    if (g == 0 && which == 0 && tid == 0) { u.norm_scratch[0] = 0.0; u.norm_scratch[1] = 0.0; }

    // Deep prefetch (three hidden layers, one output tile per wave): the weights depend on nothing, so the
    // fragments of BOTH hidden-to-hidden layers are requested before anything else; as each set is consumed
    // its registers are refilled with the dgrad fragments of the backward pass (W2 first, then W1).  Every
    // weight load is then in flight for at least two phases -- including the cold first touch after the
    // Adam kernel rewrote the bucket -- instead of one barrier.
    // (TABLES: the dgrad sets are not requested behind the forward MFMAs but where the wave's issue holds nobody up; see
    //  the hidden forward layers below.)
    const bool has_tile = HT >= kNW || wave < HT;          // waves beyond the tile count idle in MFMA phases (H < 128)
    static_assert(!TABLES || HT <= kNW, "deep prefetch: one output tile per wave");
    const bool deep = TABLES || (depth == 3 && HT <= kNW);   // (TABLES: the caller has checked depth == 3)
    float4 fr[HT], fr2[HT];
    // first layer with at most 16 inputs: its 4 weight values per lane are requested early as well
    const bool l0_pre = in_dim <= 16 && HT <= kNW && has_tile;
    float l0w[4] = {0.f, 0.f, 0.f, 0.f};
    float l2_touch = 0.f;
    // biases and output-layer weights: requested into registers now, stored to LDS after the row loads
    // below have been issued too -- one wait covers all of them (a store in between would serialise
    // the cold misses: this bucket was rewritten by the Adam kernel a moment ago)
    constexpr int kCopyRegs = 4;                          // (depth + 1) * H and out_dim * H are <= 4 * threads
    float bias_reg[kCopyRegs], wout_reg[kCopyRegs];
    const int n_bias = (depth + 1) * H, n_wout = out_dim * H;
    const bool copy_fits = n_bias <= kCopyRegs * kThreadsU && n_wout <= kCopyRegs * kThreadsU;
    auto request_weights = [&]() {
        // (fr, fr2 stay captured here though only request_hidden_sets fills them: without the two captures six fwd_bwd
        //  kernels, <8,8,*> among them, come out with other register numbers and one more SGPR spill)
        (void)fr; (void)fr2;
        // request order = arrival order (a wave's loads return in order) -- layer 0's operands, biases and output weights
        // go out BEFORE the 2 x 8 KB per wave of hidden-layer sets, so the first layer starts after one memory round trip
        // instead of behind the whole stream (round 4)
        if (l0_pre) {
            const float* w = P + offW(0) + (long)(wave * 16 + (lane & 15)) * in_dim;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int k = 4 * j + (lane >> 4); if (k < in_dim) l0w[j] = w[k]; }
        }
        // The weights were rewritten by the Adam kernel a moment ago, so this XCD's L2 does not hold them:
        // the first touch of every 128-B line of the network is requested here, before anything else, so
        // the misses overlap the index / gather / first-layer phases instead of stalling the hidden layers.
        // Not for 256-wide networks: the touches pull the whole 786 KB network through the CU's 64 B/clk vector L1 a third
        // time (after them the forward and the dgrad fragments), and every load of the prologue queues behind them (vmcnt
        // retires in order): critic workgroup 103 k -> 93 k cycles without them (stamps), hidden forward unchanged.
#ifndef PPOAF_L2_TOUCH_MAX_HT
#define PPOAF_L2_TOUCH_MAX_HT 8
#endif
        if (!deep && HT <= PPOAF_L2_TOUCH_MAX_HT) for (long i = (long)tid * 32; i < nd.size; i += (long)kThreadsU * 32) l2_touch += P[i];
        if (copy_fits) {
#pragma unroll
            for (int r = 0; r < kCopyRegs; ++r) {
                const int i = tid + r * kThreadsU;
                bias_reg[r] = 0.f; wout_reg[r] = 0.f;
                if (i < n_bias) { const int l = i / H, j = i - l * H; if (l < depth || j < out_dim) bias_reg[r] = P[offB(l) + j]; }
                if (i < n_wout) wout_reg[r] = P[offW(depth) + i];
            }
        }
    };
    // ... and the hidden sets, LAST of the prologue's requests: whatever a wave asks for behind them arrives behind 16 KB
    auto request_hidden_sets = [&]() {
        if (deep && has_tile) {
            load_fwd_lines_buf<HT>(P + offW(1), wave * 16, lane, fr);
            load_fwd_lines_buf<HT>(P + offW(2), wave * 16, lane, fr2);
        }
    };
    // the weights first (cold misses, nothing to wait for)
    // per-epoch tables in shuffled order: an input row's address depends on the cursor only -- requested now (16 x in_dim <=
    // 1024 values: two per thread), dropped below where the row turns out to be padding
    const float* x_src = which == 0 ? u.obs : u.critic_obs;
    const bool x_pre = (TABLES || u.pregathered) && kRows * in_dim <= 2 * kThreadsU;
    float xr[2] = {0.f, 0.f};
    if (x_pre) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + q * kThreadsU;
            if (idx < kRows * in_dim && (long)g * kRows + idx / in_dim < B) xr[q] = x_src[(base + (long)g * kRows) * in_dim + idx];
        }
    }
    // (a line of text in the assembly: tools/prologue_isa.py reads the TABLES flavour's prologue from here)
    if constexpr (TABLES) asm volatile("; ppoaf_rowtile_tables_prologue");
    request_weights();

    // Wave 0's row lanes and the statistics lane, in arrival order as well (a wave's loads retire in order): with the
    // per-epoch tables in shuffled order (u.pregathered) the address of a row's scalars -- like the index itself -- depends
    // on the cursor only, so they are requested HERE, ahead of the hidden sets, and consumed below where they always were.
    // Behind the sets, the index alone cost wave 0 the arrival of its whole 16 KB of W_1 / W_2 before layer 0 could start,
    // and the scalars a further round trip after that.  Outside the TABLES flavour the scalars keep their dependent trip.
    constexpr int kActRegs = 8;                            // sActF holds 8 action words per row
    constexpr int kVnPre = 2;                              // per-rank value-normaliser records requested ahead of the sets
    const bool row_lane = tid < kRows && (long)g * kRows + tid < B;      // rows >= B: no address is formed
    constexpr bool early = TABLES;                         // (every other case: behind the index, as it was)
    const int n_act = which != 0 ? 0 : head_kind_as<HEAD>(u) == PPOAF_HEAD_CATEGORICAL ? 1
                    : head_kind_as<HEAD>(u) == PPOAF_HEAD_MULTI_CATEGORICAL ? u.n_slices : out_dim;
    long perm_v = -1;
    float av = 0.f, lpo = 0.f, rt = 0.f;
    int act_bits[kActRegs];                                // raw actions as sActF keeps them: class indices, or float bits
#pragma unroll
    for (int j = 0; j < kActRegs; ++j) act_bits[j] = 0;
    auto request_row_scalars = [&](const long di) {
        if (which == 0) {
            av = u.adv[di]; lpo = u.old_lp[di];
            if (head_kind_as<HEAD>(u) == PPOAF_HEAD_CATEGORICAL) {
                act_bits[0] = (int)reinterpret_cast<const int64_t*>(u.raw_actions)[di];
            } else if (head_kind_as<HEAD>(u) == PPOAF_HEAD_MULTI_CATEGORICAL) {
#pragma unroll
                for (int j = 0; j < kActRegs; ++j)
                    if (j < n_act) act_bits[j] = (int)reinterpret_cast<const int64_t*>(u.raw_actions)[(long)di * u.n_slices + j];
            } else {
#pragma unroll
                for (int d = 0; d < kActRegs; ++d)
                    if (d < n_act) act_bits[d] = __float_as_int(reinterpret_cast<const float*>(u.raw_actions)[(long)di * out_dim + d]);
            }
        } else {
            rt = u.rtg[di];
        }
    };
    if (row_lane) {
        const long s = (long)g * kRows + tid;
        perm_v = u.perm[base + s];
        if (early) request_row_scalars(base + s);
    }
    // the statistics lane's words: the mini-batch's advantage record, or the value normaliser's state and the first
    // kVnPre per-rank records of the mini-batch (ranks beyond them are read in the merge loop below)
    const bool stat_lane = tid == 64;
    double adv_rec[3] = {0.0, 0.0, 0.0}, vn_rec[kVnPre][3];
    float vn_m = 0.f, vn_v = 0.f;
    double vn_cnt = 0.0;
#pragma unroll
    for (int r = 0; r < kVnPre; ++r) { vn_rec[r][0] = 0.0; vn_rec[r][1] = 0.0; vn_rec[r][2] = 0.0; }
    if (stat_lane) {
        if (which == 0) {
            if (u.normalize_adv) {
                const double* rec = u.adv_records + mb * 3;
                adv_rec[0] = rec[0]; adv_rec[1] = rec[1]; adv_rec[2] = rec[2];
            }
        } else {
            const int slot = (int)(mb & 1);
            vn_m = u.vn_mean[slot]; vn_v = u.vn_var[slot];
            vn_cnt = u.vn_count[slot];
            if (u.normalize_values) {
#pragma unroll
                for (int r = 0; r < kVnPre; ++r) {
                    if (r < u.n_ranks) {
                        const double* rec = u.vn_records + (mb * u.n_ranks + r) * 3;
                        vn_rec[r][0] = rec[0]; vn_rec[r][1] = rec[1]; vn_rec[r][2] = rec[2];
                    }
                }
            }
        }
    }
    // Chan merge of the per-rank records of this mini-batch (one step; the reference's order: rank 0 first)
    // (chan_merge of running_stats_device.hpp, written out: calling it here renumbers registers in these kernels)
    double vn_n = 0.0, vn_bm = 0.0, vn_M2 = 0.0;
    auto vn_merge = [&](const double nb, const double mean, const double m2) {
        if (nb <= 0.0) return;
        const double d = mean - vn_bm, nn = vn_n + nb;
        vn_bm += d * (nb / nn);
        vn_M2 += m2 + d * d * vn_n * nb / nn;
        vn_n = nn;
    };
    // more ranks than records requested above: their reads depend on nothing but the cursor either, but somebody has to
    // hold them -- merged here, one dependent trip of this lane's wave ahead of its sets, so that no wait behind the sets
    // ever waits for a set
    if (stat_lane && which != 0 && u.normalize_values && u.n_ranks > kVnPre) {
#pragma unroll
        for (int r = 0; r < kVnPre; ++r) vn_merge(vn_rec[r][0], vn_rec[r][1], vn_rec[r][2]);
        for (int r = kVnPre; r < u.n_ranks; ++r) {
            const double* rec = u.vn_records + (mb * u.n_ranks + r) * 3;
            vn_merge(rec[0], rec[1], rec[2]);
        }
    }
    request_hidden_sets();

    if (tid < kRows) {
        auto store_row = [&](const int row, const bool have) {
            if (have) {
#pragma unroll
                for (int j = 0; j < kActRegs; ++j)
                    if (j < n_act) reinterpret_cast<int*>(sActF)[tid * 8 + j] = act_bits[j];
            }
            sRow[tid] = row;
            sRowF[tid] = av; sRowF[16 + tid] = lpo; sRowF[32 + tid] = rt;
        };
        if constexpr (TABLES) {
            // everything this lane stores was requested ahead of the sets
            int row = -1;
            if (row_lane && perm_v >= 0 && perm_v < u.n_rows) row = (int)perm_v;
            store_row(row, row_lane);
        } else {
            int row = -1;
            long di = -1;                                  // where this row's inputs are read from
            if (row_lane) {
                const long p = perm_v;
                if (p >= 0 && p < u.n_rows) row = u.row_map ? u.row_map[p] : (int)p;
                di = u.pregathered ? base + (long)g * kRows + tid : row;
            }
            if (di >= 0 && !early) request_row_scalars(di);
            store_row(row, di >= 0);
        }
    }

    // ---- S0: everything that does not depend on the rows is requested first: rows / statistics,
    //      biases + output weights -> LDS, and this wave's first-layer weight fragments -> registers.
    if (stat_lane) {                                        // a lane of wave 1: mini-batch statistics
        if (which == 0) {
            float mean_f = 0.f, std_f = 1.f;
            if (u.normalize_adv) adv_mean_std(adv_rec, mean_f, std_f);     // from the per-epoch table
            sMisc[0] = mean_f; sMisc[1] = std_f;
        } else {
            const int slot = (int)(mb & 1);
            float m = vn_m, v = vn_v;
            double cnt = vn_cnt;
            if (u.normalize_values) {
                // the records requested ahead of the sets (unless the dependent trip above has merged them already), then
                // the reference's integrate (running_integrate, written out for the same reason as the merge above)
                if (u.n_ranks <= kVnPre) {
#pragma unroll
                    for (int r = 0; r < kVnPre; ++r)
                        if (r < u.n_ranks) vn_merge(vn_rec[r][0], vn_rec[r][1], vn_rec[r][2]);
                }
                const double n = vn_n, bm = vn_bm, M2 = vn_M2;
                if (n > 0.0) {
                    const float batch_mean = (float)bm, batch_var = (float)(M2 / n);
                    const float delta = batch_mean - m;
                    const double new_count = cnt + n;
                    const float new_mean = (float)((double)m + (double)delta * (n / new_count));
                    const double m_2 = (double)v * cnt + (double)batch_var * n +
                                       (double)(delta * delta) * cnt * n / (cnt + n);
                    m = new_mean; v = (float)(m_2 / (cnt + n)); cnt = new_count;
                }
            }
            sMisc[2] = m; sMisc[3] = v;
            if (g == 0) { u.vn_mean[slot ^ 1] = m; u.vn_var[slot ^ 1] = v; u.vn_count[slot ^ 1] = cnt; }
        }
    }
    if (copy_fits) {
#pragma unroll
        for (int r = 0; r < kCopyRegs; ++r) {
            const int i = tid + r * kThreadsU;
            if (i < n_bias) sBias[i] = bias_reg[r];
            if (i < n_wout) sWout[i] = wout_reg[r];
        }
    } else {
        for (int l = 0; l <= depth; ++l) {
            const int n = (l == depth) ? out_dim : H;
            const float* bb = P + offB(l);
            for (int i = tid; i < n; i += kThreadsU) sBias[l * H + i] = bb[i];
        }
        for (int i = tid; i < out_dim * H; i += kThreadsU) sWout[i] = P[offW(depth) + i];
    }
    for (int i = tid; i < kRows * INP; i += kThreadsU) sX[i] = 0.f;
    __syncthreads();
    PPOAF_STAMP(1);

    // ---- S1: gather the input rows (K4)
    if (x_pre) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + q * kThreadsU;
            const int s = idx / in_dim, i = idx - s * in_dim;
            if (idx < kRows * in_dim && sRow[s] >= 0) sX[s * INP + i] = xr[q];
        }
    } else {
        const float* src = x_src;
        for (int idx = tid; idx < kRows * in_dim; idx += kThreadsU) {
            const int s = idx / in_dim, i = idx - s * in_dim;
            const int row = sRow[s];
            const long di = (TABLES || u.pregathered) ? base + (long)g * kRows + s : row;
            if (row >= 0) sX[s * INP + i] = src[di * in_dim + i];
        }
    }
    // prefetch: fragments of the first hidden-to-hidden layer (or nothing if depth == 1)
    if (!deep && depth > 1 && has_tile) load_fwd_lines_buf<HT>(P + offW(1), wave * 16, lane, fr);
    __syncthreads();
    PPOAF_STAMP(2);
    if constexpr (SPLIT && XLD) {      // ... zero padded to the panel's stride, 64 .. 512 columns (a power of two, uniform per network)
        const int xld = u.sp.xld[which], sh = __builtin_ctz((unsigned)xld);
        float* xb = u.sp.xbuf[which] + (long)g * kRows * xld;
        for (int i = tid; i < kRows * xld; i += kThreadsU) {
            const int r = i >> sh, c = i & (xld - 1);
            xb[i] = c < 16 * NT0 ? sX[r * INP + c] : 0.f;
        }
    } else if (SPLIT) {     // the block's input rows, zero padded to 64 columns: the layer-0 wgrad's K-panel
        float* xb = u.sp.xbuf[which] + (long)g * kRows * 64;
        for (int i = tid; i < kRows * 64; i += kThreadsU) {
            const int r = i >> 6, c = i & 63;
            xb[i] = c < 16 * NT0 ? sX[r * INP + c] : 0.f;
        }
    }

    // ---- L0: first layer on MFMA, K = in_dim padded to a multiple of 4 (sX is zero padded)
    for (int nt = wave; nt < HT; nt += kNW) {
        const int o = nt * 16 + (lane & 15);
        const float bv = sBias[o];
        f32x4 acc = {bv, bv, bv, bv};
        const float* w = P + offW(0) + (long)o * in_dim;
        const float* arow = sX + (lane & 15) * INP;
        for (int k0 = 0; k0 < in_dim; k0 += 16) {            // 4 MFMA steps per 16 input columns
            float bq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * j + (lane >> 4);
                bq[j] = l0_pre ? l0w[j] : (k < in_dim ? w[k] : 0.f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sH[(4 * (lane >> 4) + r) * HS + o] = act_fwd_as<ACT>(acc[r], act);
    }
    __syncthreads();
    PPOAF_STAMP(3);

    // ---- hidden layers forward; the next phase's fragments are requested before each barrier
    // (lines of text in the assembly: tools/prologue_isa.py reads the TABLES flavour's hidden layers between them)
    if constexpr (TABLES) asm volatile("; ppoaf_rowtile_hidden_fwd_begin" ::: "memory");
    for (int l = 1; l < depth; ++l) {
        if constexpr (TABLES) asm volatile("; ppoaf_rowtile_hidden_layer_begin" ::: "memory");
        const float* Hp = sH + (long)(l - 1) * kRows * HS;
        float* Hc = sH + (long)l * kRows * HS;
        if (SPLIT) publish_begin(Hp, u.sp.hbuf[which] + (long)(l - 1) * sp_plane);     // h_{l-1}: the K-panel of dW_l
        PPOAF_HSTAMP(0);
        if constexpr (TABLES) {
            // One output tile per wave, and no request for a dgrad set behind the layer's MFMAs: a wave issues in order, and
            // 32 value-by-value loads per wave between the MFMAs and the epilogue stood in front of the layer's barrier.
            // Waves 1-7 ask where they are parked anyway (below: the output layer, the head); wave 0 runs the head, so it
            // asks through its own MFMA loops, where nobody else is loading.
            if (has_tile) {
                const int o = wave * 16 + (lane & 15);
                const float bv = sBias[l * H + o];
                f32x4 acc;
                if (wave == 0) {
                    if (l == 1) acc = mfma_rows_x_lines_paced<HT>(Hp, HS, lane, fr, bv, sScr, P + offW(2), wave * 16);
                    else acc = mfma_rows_x_lines_paced<HT>(Hp, HS, lane, fr2, bv, sScr, P + offW(1), wave * 16);
                } else {
                    acc = l == 1 ? mfma_rows_x_lines<HT>(Hp, HS, lane, fr, bv, sScr) : mfma_rows_x_lines<HT>(Hp, HS, lane, fr2, bv, sScr);
                }
                PPOAF_HSTAMP(1);
#pragma unroll
                for (int r = 0; r < 4; ++r) Hc[(4 * (lane >> 4) + r) * HS + o] = act_fwd_as<ACT>(acc[r], act);
                asm volatile("; ppoaf_rowtile_hidden_epilogue_end" ::: "memory");
            }
            if (SPLIT) publish_end(u.sp.hbuf[which] + (long)(l - 1) * sp_plane);
            PPOAF_HSTAMP(3);
            PPOAF_HSTAMP(2);
        } else {
        for (int nt = wave; nt < HT; nt += kNW) {
            const int o = nt * 16 + (lane & 15);
            f32x4 acc;
            if (deep) {
                if (l == 1) {
                    acc = mfma_rows_x_lines<HT>(Hp, HS, lane, fr, sBias[l * H + o], sScr);
                    load_dgrad_frags<HT>(P + offW(2), wave * 16, lane, fr);  // first backward phase, two phases early
                } else {
                    acc = mfma_rows_x_lines<HT>(Hp, HS, lane, fr2, sBias[l * H + o], sScr);
                    load_dgrad_frags<HT>(P + offW(1), wave * 16, lane, fr2); // second backward phase
                }
            } else {
            if (nt != wave) load_fwd_lines_buf<HT>(P + offW(l), nt * 16, lane, fr);
            acc = mfma_rows_x_lines<HT>(Hp, HS, lane, fr, sBias[l * H + o], sScr);
            if (nt + kNW >= HT) {                           // last tile of this wave in this layer
                if (l + 1 < depth) load_fwd_lines_buf<HT>(P + offW(l + 1), wave * 16, lane, fr);
                else load_dgrad_frags<HT>(P + offW(l), wave * 16, lane, fr);   // first backward phase
            }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Hc[(4 * (lane >> 4) + r) * HS + o] = act_fwd_as<ACT>(acc[r], act);
        }
        if (SPLIT) publish_end(u.sp.hbuf[which] + (long)(l - 1) * sp_plane);
        }
        __syncthreads();
        PPOAF_HSTAMP(4);
        PPOAF_HSTAMP_FLUSH(l - 1);
    }
    PPOAF_STAMP(4);
    const float* Hlast = sH + (long)(depth - 1) * kRows * HS;

    // ---- output layer (out_dim <= 8): VALU from LDS + 16-lane reductions
    if constexpr (TABLES) {                            // waves 4-7 have nothing to do in this phase: both their dgrad sets
        if (has_tile && wave >= 4) {
            load_dgrad_frags<HT>(P + offW(2), wave * 16, lane, fr);
            load_dgrad_frags<HT>(P + offW(1), wave * 16, lane, fr2);
        }
    }
    if (tid < 256) {
        const int s = tid >> 4, part = tid & 15;
        for (int k = 0; k < out_dim; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < HT; ++i) acc = fmaf(Hlast[s * HS + part + 16 * i], sWout[k * H + part + 16 * i], acc);
            acc = group16_sum(acc);
            if (part == 0) sOut[s * kMaxOut + k] = acc + sBias[depth * H + k];
        }
    }
    __syncthreads();
    PPOAF_STAMP(5);

    // ---- distribution head + loss terms for this workgroup's rows (K6 + K3): the row part only -- d loss / d out is what
    //      the backward pass waits for.  The block's loss partials and the critic's values leave at the end of the body.
    if (wave == 0) {
        if constexpr (TABLES) asm volatile("; ppoaf_rowtile_head_rows_begin");
        ppo_head_rows<HEAD>(u, which, out_dim, P + nd.log_std_off, sRow, sRowF, sMisc, sActF, sOut, sDOut, lane, B);
        if constexpr (TABLES) asm volatile("; ppoaf_rowtile_head_rows_end");
        PPOAF_STAMP_W(0, 0);
    }
    if constexpr (TABLES) {                            // waves 1-3 are parked at the barrier below while wave 0 runs the head
        if (has_tile && wave >= 1 && wave < 4) {
            load_dgrad_frags<HT>(P + offW(2), wave * 16, lane, fr);
            load_dgrad_frags<HT>(P + offW(1), wave * 16, lane, fr2);
        }
    }
    __syncthreads();
    if constexpr (TABLES) asm volatile("; ppoaf_rowtile_middle_begin");
    PPOAF_STAMP(6);

    // ---- output layer backward, the part the hidden backward waits for: dz_last = (dOut . W_out) * act'(Hlast), on all
    //      eight waves -- 16 rows x 32 lane groups of H / 32 adjacent columns (weights from LDS; every element adds its
    //      out_dim products in the order k = 0, 1, ...).  Nothing between the two barriers touches global memory.
    {
        constexpr int CP = H / 32;
        static_assert(kThreadsU == 32 * kRows && H % 32 == 0, "dz_last: 32 lane groups per row");
        const int s = tid >> 5, c0 = (tid & 31) * CP;
        float d[8];
        const float4 d0 = *reinterpret_cast<const float4*>(sDOut + s * kMaxOut);
        const float4 d1 = *reinterpret_cast<const float4*>(sDOut + s * kMaxOut + 4);
        d[0] = d0.x; d[1] = d0.y; d[2] = d0.z; d[3] = d0.w; d[4] = d1.x; d[5] = d1.y; d[6] = d1.z; d[7] = d1.w;
        float hv[CP], acc[CP], wv[CP];
        lds_read_adjacent<CP>(Hlast + s * HS + c0, hv);
#pragma unroll
        for (int ii = 0; ii < CP; ++ii) acc[ii] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < out_dim) {
                lds_read_adjacent<CP>(sWout + k * H + c0, wv);
#pragma unroll
                for (int ii = 0; ii < CP; ++ii) acc[ii] = fmaf(d[k], wv[ii], acc[ii]);
            }
        }
#pragma unroll
        for (int ii = 0; ii < CP; ++ii) acc[ii] = acc[ii] * act_bwd_as<ACT>(hv[ii], act);
        lds_write_adjacent<CP>(sD0 + s * HS + c0, acc);
    }
    PPOAF_STAMP_W(2, 0); PPOAF_STAMP_W(3, 4); PPOAF_STAMP_W(4, 5);
    if constexpr (TABLES) asm volatile("; ppoaf_rowtile_middle_end");
    __syncthreads();
    PPOAF_STAMP(7);
    if constexpr (TABLES) asm volatile("; ppoaf_rowtile_hidden_bwd_begin" ::: "memory");

    // ---- hidden layers backward: wgrad + bias grad + dgrad; `fr` holds this wave's dgrad fragments
    float* Dc = sD0;
    float* Dn = sD1;
    for (int l = depth - 1; l >= 1; --l) {
        const float* Hin = sH + (long)(l - 1) * kRows * HS;
        if (SPLIT) publish_begin(Dc, u.sp.dbuf[which] + (long)l * sp_plane);           // dz_l: the other panel of dW_l, db_l
        // dgrad first (its operands were prefetched): dh[s][i] = sum_o dz[s][o] * W[o][i]
        for (int nt = wave; nt < HT; nt += kNW) {
            f32x4 acc;
            if (deep) {
                acc = l == 2 ? mfma_rows_x_frags<HT>(Dc, HS, lane, fr, 0.f) : mfma_rows_x_frags<HT>(Dc, HS, lane, fr2, 0.f);
            } else {
            if (nt != wave) load_dgrad_frags<HT>(P + offW(l), nt * 16, lane, fr);
            acc = mfma_rows_x_frags<HT>(Dc, HS, lane, fr, 0.f);
            if (nt + kNW >= HT && l - 1 >= 1) load_dgrad_frags<HT>(P + offW(l - 1), wave * 16, lane, fr);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 4 * (lane >> 4) + r, i = nt * 16 + (lane & 15);
                Dn[s * HS + i] = acc[r] * act_bwd_as<ACT>(Hin[s * HS + i], act);
            }
        }
        if (SPLIT) publish_end(u.sp.dbuf[which] + (long)l * sp_plane);
        if (l == depth - 1) PPOAF_STAMP(10);
        // wgrad: dW[o][i] = sum_s dz[s][o] * Hin[s][i]   (SPLIT: left to the wgrad launch, over all rows at once)
        if (!SPLIT) {
            for (int mt = wave; mt < HT; mt += kNW) {
                if (HT <= 8) wgrad_mtile_full<(HT <= 8 ? HT : 1)>(Dc, HS, Hin, HS, mt * 16, lane, slab + offW(l), H);
                else wgrad_mtile(Dc, HS, Hin, HS, mt * 16, HT, H, lane, slab + offW(l), H);
            }
            if (l == depth - 1) PPOAF_STAMP(11);
            for (int o = tid; o < H; o += kThreadsU) {
                float acc = 0.f;
#pragma unroll
                for (int s = 0; s < kRows; ++s) acc += Dc[s * HS + o];
                slab[offB(l) + o] = acc;
            }
        }
        if (l == depth - 1) PPOAF_STAMP(12);
        __syncthreads();
        if (l == depth - 1) PPOAF_STAMP(13);
        float* t = Dc; Dc = Dn; Dn = t;
    }
    PPOAF_STAMP(8);

    // ---- first layer backward: dW0[o][i] = sum_s dz0[s][o] * x[s][i] on MFMA against the padded sX
    if (SPLIT) {
        publish_read(Dc);                                     // dz_0 (its K-panel is x, published after the gather)
        publish_store(u.sp.dbuf[which]);
    } else {
        for (int mt = wave; mt < HT; mt += kNW)
            wgrad_mtile(Dc, HS, sX, INP, mt * 16, NT0, in_dim, lane, slab + offW(0), in_dim);
        for (int o = tid; o < H; o += kThreadsU) {
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc += Dc[s * HS + o];
            slab[offB(0) + o] = acc;
        }
    }
    PPOAF_STAMP_W(6, 0);

    // ---- what nothing inside this launch consumes, last: the output layer's weight / bias gradients and the Gaussian
    //      head's d / d log_std column sums (-> the slab, or the block's row of the output partials), the block's loss
    //      partials and the critic's values.  Hlast, sDOut, sOut, sRow and the terms parked in sActF are as the middle of
    //      the body left them.  (Measured against running it behind the dgrad MFMAs of the first hidden-backward layer,
    //      where it delays that layer's barrier: profiles/middle_phase_stamps_C2.txt.)
    //      Operands are pulled into registers with independent LDS reads first; a read-per-FMA loop is LDS-latency bound
    //      (~64 cycles each).  (dW_out as one element per thread over all eight waves measured slower: same file.)
    if (tid < H) {
        const int i = tid;
        float h[kRows];
#pragma unroll
        for (int s = 0; s < kRows; ++s) h[s] = Hlast[s * HS + i];
        for (int k = 0; k < out_dim; ++k) {
            float d[kRows];
#pragma unroll
            for (int s = 0; s < kRows; ++s) d[s] = sDOut[s * kMaxOut + k];
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc = fmaf(d[s], h[s], acc);
            slab[offW(depth) + (long)k * H + i] = acc;
        }
    }
    {
        // (SPLIT: the padding slots of the segment are written too, as zeros -- the partials row lives in a workspace whose
        //  layout changes with the mini-batch size, so nothing in it may be assumed to be zero; a slab's padding is never touched)
        const int out_pad = SPLIT ? ((out_dim + 3) & ~3) : out_dim;
        if (tid >= 256 && tid < 256 + out_pad) {
            const int k = tid - 256;
            float acc = 0.f;
            if (k < out_dim) {
#pragma unroll
                for (int s = 0; s < kRows; ++s) acc += sDOut[s * kMaxOut + k];
            }
            slab[offB(depth) + k] = acc;
        }
        if (which == 0 && head_kind_as<HEAD>(u) == PPOAF_HEAD_GAUSSIAN && tid >= 320 && tid < 320 + out_pad) {
            const int d = tid - 320;
            float acc = 0.f;
            if (d < out_dim) {
#pragma unroll
                for (int s = 0; s < kRows; ++s) acc += sOut[s * kMaxOut + 8 + d];
            }
            slab[nd.log_std_off + d] = acc;
        }
        if (which != 0 && wave == 6) ppo_head_values(u, sRow, sOut, lane);
        if (wave == 7) ppo_head_block(u, which, g, sMisc, sActF, lane);
        PPOAF_STAMP_W(5, 0); PPOAF_STAMP_W(1, 7);
    }
    if (l2_touch == 1.2345e38f) u.loss_partials[0] = l2_touch;   // keeps the early line touches alive
    PPOAF_STAMP(9);
}

template <int HT, bool SPLIT = false, bool XLD = false>
__device__ __forceinline__ void ppo_update_fwd_bwd_body(const UpdateDev& u, const int which, const int g) {
    if constexpr (HT <= kNW) {
        if (u.net[which].depth == 3 && u.pregathered && !u.row_map) {        // uniform
            ppo_update_fwd_bwd_body_as<HT, SPLIT, true, XLD>(u, which, g);
            return;
        }
    }
    ppo_update_fwd_bwd_body_as<HT, SPLIT, false, XLD>(u, which, g);
}

// dynamic LDS the body needs for one network
constexpr size_t kRowtileLineFloats = (size_t)kNW * 2 * kLineSlot;         // the waves' line slots, behind the carve below
inline size_t rowtile_lds_floats(const NetDev& n) {
    const size_t HS = n.H + 4, INP = 16 * ((n.in_dim + 15) / 16) + 4;
    return 208 + (size_t)(n.depth + 1) * n.H + 8 * (size_t)n.H + kRows * INP + (size_t)n.depth * kRows * HS + 2 * kRows * HS +
           2 * kRows * kMaxOut;
}

}  // namespace ppoaf
