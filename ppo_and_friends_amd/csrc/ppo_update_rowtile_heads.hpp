// The row tile of a 256-wide ACTOR with 9 .. 24 outputs (kWideOut; the wide heads of the 256/512 pair: Categorical and
// tanh-Gaussian) -- K12's fwd_bwd body for that network, a body of its own beside ppo_update_rowtile.hpp's, which every
// launch with out_dim <= 8 keeps running.  The pair exists on the split-wgrad chain only, so this body is the SPLIT form
// with the layer-0 panel's stride read from the arguments (u.sp.xld); at sixteen output tiles per layer it is the plain
// flavour of the other body (no per-epoch-table prologue, no deep prefetch): forward, head, dz_last and dgrad as there,
// the same MFMA operands in the same order.
//
// LDS.  The carve is the other body's, float for float, but for the input rows: no byte is added for the wider head.
//   [0, 208)    sRow[16], sMisc[16], sRowF[3][16], sPark[16][8]: a row's loss terms for ppo_head_block (where the narrow
//               body keeps the raw actions first)
//   sBias       [(depth + 1), H]
//   sWout       [8, H]: output rows 0 .. 7
//   sX          [16, INP], at least 768 floats.  Dead once layer 0 has run (the x panel is published after the gather), so
//               from the output layer on it holds sDO[16][24], d loss / d out, and behind it sLs[16][24], the Gaussian
//               head's per-row d / d log_std.  Sixteen rows of >= 33 inputs are 768 floats already; below that the region
//               is rounded up to 768 (rowtile_heads_lds_floats), far from any LDS edge.
//   sH          depth x [16, HS]
//   sD0         [16, HS]: the raw actions [16][24] (class index or float bits) from the prologue until the head has read
//               them; dz_last writes the plane one barrier later.
//   sD1         [16, HS] = 4160 floats: output rows 8 .. 23 of W_out, [16, H] = 4096 floats, from the prologue until dz_last
//               has read them; the first hidden-backward layer writes the plane one barrier later (depth 1: never).
//   sZ          [16][24] in the 512 floats of the narrow body's sOut + sDOut: the output layer's values
//   line slots  two per wave, as there
#pragma once
#include "ppo_update_rowtile.hpp"

namespace ppoaf {

// (kHeadStride, kHeadXFloats and the host's formula rowtile_heads_lds_floats: ppo_update_dev.hpp)

// The row part of the actor's head for up to 24 outputs, run by ONE wave: ppo_head_rows' chain and gradient formulas
// (ppo_update_dev.hpp) on rows kHeadStride floats apart.  sAct: the raw actions; sZ: the output layer's values; -> sDO,
// d loss / d out (all 24 slots of every row written, zeros beyond out_dim and in dead rows), sLs, the Gaussian head's per-row
// d / d log_std, and the row's loss terms parked in sPark[16][8] for ppo_head_block.
//   Categorical: 4 lanes per row, lane (s4, q) owns the six classes q, q + 4, .. q + 20 -- six values of every per-class
//   quantity per lane, indexed by unrolled loop counters only; the class reductions are two DPP steps inside the 4-lane group.
//   Gaussian: one lane per row and the dimensions in order, so that a row's log-prob is the sum K6 logged, bit for bit.
__device__ __forceinline__ void ppo_head_rows_wide(const UpdateDev& u, const int out_dim, const float* __restrict__ log_std,
                                                   const int* sRow, const float* sRowF, const float* sMisc,
                                                   const float* sAct, float* sPark, const float* sZ, float* sDO, float* sLs,
                                                   const int lane, const long B) {
    constexpr int ST = kHeadStride, NJ = kWideOut / 4;
    const float inv_B = 1.0f / (float)B;
    const float lo = 1.0f - u.surr_clip, hi = 1.0f + u.surr_clip;
    const float gH = (u.entropy_weight != 0.0f) ? -u.entropy_weight * inv_B : 0.f;
    float part0 = 0.f, part3 = 0.f, part4 = 0.f, part7 = 0.f;
    if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
        const int s4 = lane >> 2, q = lane & 3;
        const bool live4 = sRow[s4] >= 0;
        float av4 = 0.f, lpo4 = 0.f;
        if (live4) {
            av4 = sRowF[s4]; lpo4 = sRowF[16 + s4];
            if (u.normalize_adv) av4 = (av4 - sMisc[0]) / (sMisc[1] + 1e-8f);
        }
        float z[NJ], p[NJ], n[NJ], l[NJ], gk[NJ];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            z[j] = q + 4 * j < out_dim ? sZ[s4 * ST + q + 4 * j] : -INFINITY;
            m = fmaxf(m, z[j]);
        }
        m = group4_max(m);
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { p[j] = q + 4 * j < out_dim ? expf(z[j] - m) : 0.f; t += p[j]; }
        const float inv = 1.0f / group4_sum(t);
        t = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { p[j] *= inv; t += p[j]; }
        const float s2 = group4_sum(t);                                   // Categorical's renormalisation
        int a = reinterpret_cast<const int*>(sAct)[s4 * ST];
        a = a < 0 ? 0 : (a >= out_dim ? out_dim - 1 : a);
        float te = 0.f, tl = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const bool v = q + 4 * j < out_dim;
            n[j] = p[j] / s2;
            l[j] = v ? logf(clamp_prob_u(n[j])) : 0.f;
            te += v ? n[j] * l[j] : 0.f;
            tl += q + 4 * j == a ? l[j] : 0.f;
        }
        const float ent4 = -group4_sum(te);
        const float logp4 = group4_sum(tl);
        const float ratio = expf(logp4 - lpo4);
        const float bad4 = (isnan(ratio) || isinf(ratio)) ? 1.f : 0.f;
        const float surr1 = ratio * av4, surr2 = fminf(fmaxf(ratio, lo), hi) * av4;
        float glp;
        if (surr1 <= surr2) glp = -av4 * ratio;
        else glp = (ratio >= lo && ratio <= hi) ? -av4 * ratio : 0.f;
        glp *= inv_B;
        // chain: z -softmax-> p -(/sum)-> n -clamp,log-> l
        float td = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            gk[j] = 0.f;
            if (q + 4 * j < out_dim) {
                const float ck = clamp_prob_u(n[j]);
                const float in_range = (n[j] >= FLT_EPSILON && n[j] <= 1.0f - FLT_EPSILON) ? 1.f : 0.f;
                gk[j] = gH * (-l[j] - n[j] * in_range / ck);
                if (q + 4 * j == a) gk[j] += glp * in_range / ck;
            }
            td += gk[j] * n[j];
        }
        const float dot = group4_sum(td);
        td = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { gk[j] = (gk[j] - dot) / s2; td += gk[j] * p[j]; }
        const float dot2 = group4_sum(td);
#pragma unroll
        for (int j = 0; j < NJ; ++j) sDO[s4 * ST + q + 4 * j] = live4 ? p[j] * (gk[j] - dot2) : 0.f;    // (padding classes: p = 0)
        if (live4) { part0 = -fminf(surr1, surr2); part3 = ent4; part4 = lpo4 - logp4; part7 = bad4; }
        if (q == 0) {
            float* pk = sPark + s4 * 8;
            pk[0] = part0; pk[2] = 0.f; pk[3] = part3; pk[4] = part4; pk[7] = part7;
        }
        return;
    }
    // tanh-Gaussian (distributions.py:441-694)
    const int s = lane;
    if (s >= kRows) return;
    const bool live = sRow[s] >= 0;
    if (live) {
        float av = sRowF[s];
        const float lpo = sRowF[16 + s];
        if (u.normalize_adv) av = (av - sMisc[0]) / (sMisc[1] + 1e-8f);
        const float* x = sAct + s * ST;
        float lp = 0.f, slog = 0.f, ent = 0.f;
        for (int d = 0; d < out_dim; ++d) {
            const float sd = fmaxf(softplus_u(log_std[d]), u.min_std);
            const float mu = sZ[s * ST + d];
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
        const float logp = lp - slog;
        const float ratio = expf(logp - lpo);
        if (isnan(ratio) || isinf(ratio)) part7 = 1.f;
        const float surr1 = ratio * av, surr2 = fminf(fmaxf(ratio, lo), hi) * av;
        part0 = -fminf(surr1, surr2);
        part3 = ent;
        part4 = lpo - logp;
        float glp;
        if (surr1 <= surr2) glp = -av * ratio;
        else glp = (ratio >= lo && ratio <= hi) ? -av * ratio : 0.f;
        glp *= inv_B;
        for (int d = 0; d < out_dim; ++d) {
            const float ls = log_std[d];
            const float sp = softplus_u(ls), sd = fmaxf(sp, u.min_std);
            const float mu = sZ[s * ST + d];
            const float zz = x[d] - mu;
            const float l0 = -logf(sd) - 0.91893853320467274178f;
            const float l = -(zz * zz) / (2.0f * sd * sd) + l0;
            const float pass = (l >= -100.f && l <= 100.f) ? 1.f : 0.f;
            const float pass0 = (l0 >= -100.f && l0 <= 100.f) ? 1.f : 0.f;
            const float thm = tanhf(mu);
            const float pass_t = (1.0f - thm * thm >= 1e-6f) ? 1.f : 0.f;
            sDO[s * ST + d] = glp * pass * zz / (sd * sd) - gH * pass_t * 2.0f * thm;
            const float dmax = sp > u.min_std ? 1.f : (sp == u.min_std ? 0.5f : 0.f);
            const float dsp = ls > 20.f ? 1.f : 1.0f / (1.0f + expf(-ls));
            sLs[s * ST + d] = (glp * pass * (zz * zz / (sd * sd * sd) - 1.0f / sd) + gH * pass0 / sd) * dmax * dsp;
        }
        for (int d = out_dim; d < ST; ++d) { sDO[s * ST + d] = 0.f; sLs[s * ST + d] = 0.f; }
    } else {
        for (int d = 0; d < ST; ++d) { sDO[s * ST + d] = 0.f; sLs[s * ST + d] = 0.f; }
    }
    float* pk = sPark + s * 8;
    pk[0] = part0; pk[2] = 0.f; pk[3] = part3; pk[4] = part4; pk[7] = part7;
}

template <int HT>
__device__ __forceinline__ void ppo_update_fwd_bwd_body_heads(const UpdateDev& u, const int g) {
    static_assert(HT == 16, "the wide heads belong to the 256-wide actor of the wide pair");
    constexpr int H = 16 * HT, HS = H + 4, ST = kHeadStride;
    constexpr int which = 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto& nd = u.net[which];
    const int in_dim = nd.in_dim, depth = nd.depth, out_dim = nd.out_dim, act = nd.act;
    const int NT0 = (in_dim + 15) >> 4;
    const int INP = 16 * NT0 + 4;
    const float* P = u.params + nd.offset;
    const long B = u.B;
    const long mb = u.cursor[0] + u.mb_offset;
    const long base = mb * u.batch_stride;
    // layer offsets inside the bucket, by arithmetic (see the other body)
    const long szW0 = ((long)H * in_dim + 3) & ~3L;
    auto offW = [&](int l) -> long { return l == 0 ? 0 : szW0 + H + (long)(l - 1) * (H * H + H); };
    auto offB = [&](int l) -> long {
        return l == 0 ? szW0 : offW(l) + (l < depth ? (long)H * H : (((long)out_dim * H + 3) & ~3L));
    };
    // this block's row of the output-layer partials, addressed with bucket offsets
    float* slab = u.sp.outpart[which] + (long)g * (nd.size - offW(depth)) - offW(depth);
    // 16 rows x H floats of LDS -> rows [16 g, +16) of a [Bp][H] panel (two float4 per thread; stored where they are read: the
    // register file of a 256-wide tile is full)
    constexpr int kPub = (kRows * (H / 4) + kThreadsU - 1) / kThreadsU;
    auto publish = [&](const float* src, float* panel) {
        float* dst = panel + (long)g * kRows * H;
#pragma unroll
        for (int q = 0; q < kPub; ++q) {
            const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
            if (i < kRows * (H / 4))
                *reinterpret_cast<float4*>(dst + (long)r * H + 4 * c4) = *reinterpret_cast<const float4*>(src + r * HS + 4 * c4);
        }
    };
    const long sp_plane = (long)u.sp.Bp * H;

    // ---- LDS carve (the head of this file; all offsets multiples of 16 B)
    float* smem = reinterpret_cast<float*>(ppo_update_smem);
    int* sRow = reinterpret_cast<int*>(smem);                 // [16]
    float* sMisc = smem + 16;                                 // [16]: adv mean / std
    float* sRowF = smem + 32;                                 // [3][16]: adv, old log-prob
    float* sPark = smem + 80;                                 // [16][8]: the rows' loss terms
    float* sBias = smem + 208;                                // [(depth+1), H]
    float* sWout = sBias + (depth + 1) * H;                   // [8, H]: output rows 0 .. 7
    float* sX = sWout + 8 * H;                                // [16, INP], zero padded; >= kHeadXFloats
    const int x_floats = kRows * INP > kHeadXFloats ? kRows * INP : kHeadXFloats;
    float* sH = sX + x_floats;                                // depth x [16, HS]
    float* sD0 = sH + (long)depth * kRows * HS;               // [16, HS]
    float* sD1 = sD0 + kRows * HS;                            // [16, HS]
    float* sZ = sD1 + kRows * HS;                             // [16][24] of 512 floats
    float* sScr = sZ + 2 * kRows * kMaxOut + wave * 2 * kLineSlot;   // this wave's two line slots
    float* sAct = sD0;                                        // [16][24] raw actions, until the head has read them
    float* sWhi = sD1;                                        // [16, H]: output rows 8 .. 23, until dz_last has read them
    float* sDO = sX;                                          // [16][24], from the output layer on
    float* sLs = sX + kRows * ST;                             // [16][24]

    if (g == 0 && tid == 0) { u.norm_scratch[0] = 0.0; u.norm_scratch[1] = 0.0; }

    // ---- S0: the rows' index and scalars, the mini-batch's advantage record, biases and output weights -> LDS
    const bool row_lane = tid < kRows && (long)g * kRows + tid < B;      // rows >= B: no address is formed
    if (tid < kRows) {
        int row = -1;
        long di = -1;                                         // where this row's inputs are read from
        if (row_lane) {
            const long p = u.perm[base + (long)g * kRows + tid];
            if (p >= 0 && p < u.n_rows) row = u.row_map ? u.row_map[p] : (int)p;
            di = u.pregathered ? base + (long)g * kRows + tid : row;
        }
        float av = 0.f, lpo = 0.f;
        if (di >= 0) { av = u.adv[di]; lpo = u.old_lp[di]; }
        sRow[tid] = row;
        sRowF[tid] = av; sRowF[16 + tid] = lpo; sRowF[32 + tid] = 0.f;
    }
    if (tid == 64) {                                          // a lane of wave 1: the mini-batch's advantage statistics
        float mean_f = 0.f, std_f = 1.f;
        if (u.normalize_adv) adv_mean_std(u.adv_records + mb * 3, mean_f, std_f);      // from the per-epoch table
        sMisc[0] = mean_f; sMisc[1] = std_f;
    }
    for (int l = 0; l <= depth; ++l) {
        const int n = (l == depth) ? out_dim : H;
        const float* bb = P + offB(l);
        for (int i = tid; i < n; i += kThreadsU) sBias[l * H + i] = bb[i];
    }
    for (int i = tid; i < out_dim * H; i += kThreadsU) {      // rows 0 .. 7 | rows 8 .. out_dim - 1
        const float w = P[offW(depth) + i];
        if (i < 8 * H) sWout[i] = w;
        else sWhi[i - 8 * H] = w;
    }
    for (int i = tid; i < kRows * INP; i += kThreadsU) sX[i] = 0.f;
    __syncthreads();

    // ---- S1: gather the input rows (K4) and the rows' raw actions: the class index, or out_dim floats
    const int n_act = u.head_kind == PPOAF_HEAD_CATEGORICAL ? 1 : out_dim;
    for (int idx = tid; idx < kRows * in_dim; idx += kThreadsU) {
        const int s = idx / in_dim, i = idx - s * in_dim;
        const int row = sRow[s];
        const long di = u.pregathered ? base + (long)g * kRows + s : row;
        if (row >= 0) sX[s * INP + i] = u.obs[di * in_dim + i];
    }
    for (int idx = tid; idx < kRows * n_act; idx += kThreadsU) {
        const int s = idx / n_act, j = idx - s * n_act;
        const int row = sRow[s];
        const bool in_batch = (long)g * kRows + s < B;
        const long di = u.pregathered ? base + (long)g * kRows + s : row;
        int w = 0;
        if (in_batch && di >= 0) {
            if (u.head_kind == PPOAF_HEAD_CATEGORICAL) w = (int)reinterpret_cast<const int64_t*>(u.raw_actions)[di];
            else w = __float_as_int(reinterpret_cast<const float*>(u.raw_actions)[di * out_dim + j]);
        }
        reinterpret_cast<int*>(sAct)[s * ST + j] = w;
    }
    float4 fr[HT];
    if (depth > 1) load_fwd_lines_buf<HT>(P + offW(1), wave * 16, lane, fr);
    __syncthreads();
    {   // the block's input rows, zero padded to the panel's stride (64 .. 512 columns): the layer-0 wgrad's K-panel
        const int xld = u.sp.xld[which], sh = __builtin_ctz((unsigned)xld);
        float* xb = u.sp.xbuf[which] + (long)g * kRows * xld;
        for (int i = tid; i < kRows * xld; i += kThreadsU) {
            const int r = i >> sh, c = i & (xld - 1);
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
        for (int k0 = 0; k0 < in_dim; k0 += 16) {
            float bq[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * j + (lane >> 4);
                bq[j] = k < in_dim ? w[k] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sH[(4 * (lane >> 4) + r) * HS + o] = act_fwd(acc[r], act);
    }
    __syncthreads();                                          // sX is dead from here on: sDO and sLs take its place

    // ---- hidden layers forward; the next phase's fragments are requested before each barrier
    for (int l = 1; l < depth; ++l) {
        const float* Hp = sH + (long)(l - 1) * kRows * HS;
        float* Hc = sH + (long)l * kRows * HS;
        publish(Hp, u.sp.hbuf[which] + (long)(l - 1) * sp_plane);         // h_{l-1}: the K-panel of dW_l
        for (int nt = wave; nt < HT; nt += kNW) {
            const int o = nt * 16 + (lane & 15);
            if (nt != wave) load_fwd_lines_buf<HT>(P + offW(l), nt * 16, lane, fr);
            const f32x4 acc = mfma_rows_x_lines<HT>(Hp, HS, lane, fr, sBias[l * H + o], sScr);
            if (nt + kNW >= HT) {                           // last tile of this wave in this layer
                if (l + 1 < depth) load_fwd_lines_buf<HT>(P + offW(l + 1), wave * 16, lane, fr);
                else load_dgrad_frags<HT>(P + offW(l), wave * 16, lane, fr);   // first backward phase
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Hc[(4 * (lane >> 4) + r) * HS + o] = act_fwd(acc[r], act);
        }
        __syncthreads();
    }
    const float* Hlast = sH + (long)(depth - 1) * kRows * HS;

    // ---- output layer (out_dim <= 24): VALU from LDS + 16-lane reductions
    if (tid < 256) {
        const int s = tid >> 4, part = tid & 15;
        for (int k = 0; k < out_dim; ++k) {
            const float* wk = k < 8 ? sWout + k * H : sWhi + (k - 8) * H;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < HT; ++i) acc = fmaf(Hlast[s * HS + part + 16 * i], wk[part + 16 * i], acc);
            acc = group16_sum(acc);
            if (part == 0) sZ[s * ST + k] = acc + sBias[depth * H + k];
        }
    }
    __syncthreads();

    // ---- distribution head + loss terms, the row part (wave 0); the block's loss partials leave at the end of the body
    if (wave == 0)
        ppo_head_rows_wide(u, out_dim, P + nd.log_std_off, sRow, sRowF, sMisc, sAct, sPark, sZ, sDO, sLs, lane, B);
    __syncthreads();

    // ---- output layer backward, the part the hidden backward waits for: dz_last = (dOut . W_out) * act'(Hlast), on all
    //      eight waves -- 16 rows x 32 lane groups of 8 adjacent columns; every element adds its out_dim products in the
    //      order k = 0, 1, ...  The 24 d values of a row are all a lane keeps per class: 24 + 3 x 8 registers.
    {
        constexpr int CP = H / 32;
        static_assert(kThreadsU == 32 * kRows && H % 32 == 0, "dz_last: 32 lane groups per row");
        const int s = tid >> 5, c0 = (tid & 31) * CP;
        float d[kWideOut];
        lds_read_adjacent<kWideOut>(sDO + s * ST, d);
        float hv[CP], acc[CP], wv[CP];
        lds_read_adjacent<CP>(Hlast + s * HS + c0, hv);
#pragma unroll
        for (int ii = 0; ii < CP; ++ii) acc[ii] = 0.f;
#pragma unroll
        for (int k = 0; k < kWideOut; ++k) {
            if (k < out_dim) {
                lds_read_adjacent<CP>((k < 8 ? sWout + k * H : sWhi + (k - 8) * H) + c0, wv);
#pragma unroll
                for (int ii = 0; ii < CP; ++ii) acc[ii] = fmaf(d[k], wv[ii], acc[ii]);
            }
        }
#pragma unroll
        for (int ii = 0; ii < CP; ++ii) acc[ii] = acc[ii] * act_bwd(hv[ii], act);
        lds_write_adjacent<CP>(sD0 + s * HS + c0, acc);
    }
    __syncthreads();

    // ---- hidden layers backward: dgrad; `fr` holds this wave's dgrad fragments (the weight gradients: the wgrad launch)
    float* Dc = sD0;
    float* Dn = sD1;
    for (int l = depth - 1; l >= 1; --l) {
        const float* Hin = sH + (long)(l - 1) * kRows * HS;
        publish(Dc, u.sp.dbuf[which] + (long)l * sp_plane);               // dz_l: the other panel of dW_l, db_l
        for (int nt = wave; nt < HT; nt += kNW) {
            if (nt != wave) load_dgrad_frags<HT>(P + offW(l), nt * 16, lane, fr);
            const f32x4 acc = mfma_rows_x_frags<HT>(Dc, HS, lane, fr, 0.f);
            if (nt + kNW >= HT && l - 1 >= 1) load_dgrad_frags<HT>(P + offW(l - 1), wave * 16, lane, fr);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 4 * (lane >> 4) + r, i = nt * 16 + (lane & 15);
                Dn[s * HS + i] = acc[r] * act_bwd(Hin[s * HS + i], act);
            }
        }
        __syncthreads();
        float* t = Dc; Dc = Dn; Dn = t;
    }
    publish(Dc, u.sp.dbuf[which]);                            // dz_0 (its K-panel is x, published after the gather)

    // ---- what nothing inside this launch consumes, last: the output layer's weight / bias gradients and the Gaussian
    //      head's d / d log_std column sums -> the block's row of the output partials (padding slots of the segment as
    //      zeros), and the block's loss partials.  Hlast, sDO, sLs, sRow and sPark are as the middle of the body left them.
    if (tid < H) {
        const int i = tid;
        float h[kRows];
#pragma unroll
        for (int s = 0; s < kRows; ++s) h[s] = Hlast[s * HS + i];
        for (int k = 0; k < out_dim; ++k) {
            float d[kRows];
#pragma unroll
            for (int s = 0; s < kRows; ++s) d[s] = sDO[s * ST + k];
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc = fmaf(d[s], h[s], acc);
            slab[offW(depth) + (long)k * H + i] = acc;
        }
    }
    {
        const int out_pad = (out_dim + 3) & ~3;
        if (tid >= 256 && tid < 256 + out_pad) {
            const int k = tid - 256;
            float acc = 0.f;
            if (k < out_dim) {
#pragma unroll
                for (int s = 0; s < kRows; ++s) acc += sDO[s * ST + k];
            }
            slab[offB(depth) + k] = acc;
        }
        if (u.head_kind == PPOAF_HEAD_GAUSSIAN && tid >= 320 && tid < 320 + out_pad) {
            const int d = tid - 320;
            float acc = 0.f;
            if (d < out_dim) {
#pragma unroll
                for (int s = 0; s < kRows; ++s) acc += sLs[s * ST + d];
            }
            slab[nd.log_std_off + d] = acc;
        }
        if (wave == 7) ppo_head_block(u, which, g, sMisc, sPark, lane);
    }
}

}  // namespace ppoaf
