// The row-tiled forward + backward of one 16-row block of a 512-wide CRITIC (K12's fwd_bwd kernel, width pair 256/512;
// ppo_update_wide.hip).  The body of ppo_update_rowtile.hpp keeps depth + 2 activation planes in LDS and a whole K = H
// fragment set per accumulator chain in registers: at H = 512 that is 165 KB at depth 3 and the whole register file.  This
// body covers less and keeps less:
//
//   * the critic only (one output, the value head and value loss of ppo_head_rows) on the split-wgrad chain only: like the
//     SPLIT form of the other body it publishes its 16 rows of x, of every h_l and of every dLoss/dz_l (u.sp) and its row of
//     the output layer's partials, and computes no weight gradient of a hidden layer.  ppo_update_wgrad_kernel<256, 512>
//     and ppoaf_ppo_update_adam(3) consume them as they are.  No slab form, no fused tail, no workgroup pairs.
//   * three planes of 16 x (H + 4) floats.  The forward ping-pongs X0 / X1 (h_l in X[l & 1]) and publishes every h_l that
//     a weight gradient needs.  The backward keeps dz_l and dz_{l-1} in two planes and stages h_{l-1}, which act' needs,
//     into the third from the workgroup's OWN 16 rows of the hbuf panel, behind the layer's MFMAs (why behind: at the
//     loads).
//   * K in two chunks of 256: 16 float4 fragments per accumulator chain, two sets in flight (the set of step s + 1 is
//     requested before the MFMAs of step s; a step = one output tile x one K chunk, eight steps per wave and layer: wave w
//     owns output tiles w, w + 8, w + 16, w + 24).  Sums: (bias + chunk 0's two chains) + (chunk 1's two chains).
//     Fragment-shaped loads, not whole lines: the waves' line slots (36 KB) do not fit beside three planes at depth 7.
//
// One workgroup of kThreadsU threads per tile.  Nothing here waits for another workgroup: no records, no flags, no polling;
// the only synchronisation is __syncthreads() under workgroup-uniform control flow (depth, l and the step numbers are
// uniform), and the kernel's `g >= n_wg` return lies ahead of the first barrier.
#pragma once
#include "ppo_update_rowtile.hpp"

namespace ppoaf {

constexpr int kWideHT = 32;                               // 512 / 16
constexpr int kWideKC = 16;                               // MFMA chunks (of 16 k) per K chunk: 256 k
constexpr int kWideNCH = kWideHT / kWideKC;               // K chunks per output tile
constexpr int kWideSteps = kWideNCH * (kWideHT / kNW);    // (output tile, K chunk) steps of a wave per layer

__device__ __forceinline__ void ppo_update_wide_critic_body(const UpdateDev& u, const int g) {
    constexpr int which = 1;
    constexpr int HT = kWideHT, H = 16 * HT, HS = H + 4, KC = kWideKC, KW = 16 * KC;
    constexpr int NCH = kWideNCH;
    static_assert(kThreadsU == H && kThreadsU == 32 * kRows && HT % kNW == 0 && HT == NCH * KC && kWideSteps % 2 == 0, "wide body: 512 threads, 512 columns");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto& nd = u.net[which];
    const int in_dim = nd.in_dim, depth = nd.depth, act = nd.act;
    const int NT0 = (in_dim + 15) >> 4;                    // 16-column tiles of the input
    const int INP = 16 * NT0 + 4;
    const float* P = u.params + nd.offset;
    const long B = u.B;
    const long mb = u.cursor[0] + u.mb_offset;
    const long base = mb * u.batch_stride;
    const long szW0 = ((long)H * in_dim + 3) & ~3L;
    auto offW = [&](int l) -> long { return l == 0 ? 0 : szW0 + H + (long)(l - 1) * (H * H + H); };
    auto offB = [&](int l) -> long { return l == 0 ? szW0 : offW(l) + (l < depth ? (long)H * H : (long)H); };   // (W_out: one row of H)
    // this block's row of the output-layer partials, addressed with bucket offsets (as the SPLIT form of the other body)
    float* outrow = u.sp.outpart[which] + (long)g * (nd.size - offW(depth)) - offW(depth);
    const long sp_plane = (long)u.sp.Bp * H;

    // ---- LDS carve (all offsets multiples of 16 B; host: rowtile_wide_lds_floats, ppo_update_dev.hpp)
    float* smem = reinterpret_cast<float*>(ppo_update_smem);
    int* sRow = reinterpret_cast<int*>(smem);                 // [16]
    float* sMisc = smem + 16;                                 // [16]: vn mean / var at [2], [3]
    float* sRowF = smem + 32;                                 // [3][16]: -, -, rewards-to-go
    float* sActF = smem + 80;                                 // [16][8]: the rows' parked loss terms
    float* sBias = smem + 208;                                // [(depth+1), H]
    float* sWout = sBias + (depth + 1) * H;                   // [H]
    float* sX = sWout + H;                                    // [16, INP], zero padded
    float* sP0 = sX + kRows * INP;                            // three planes [16, HS]
    float* sP1 = sP0 + kRows * HS;
    float* sP2 = sP1 + kRows * HS;
    float* sOut = sP2 + kRows * HS;                           // [16, 16]
    float* sDOut = sOut + kRows * kMaxOut;                    // [16, 16]

    // 16 rows x H floats of a plane <-> rows [16 g, +16) of a [Bp][H] panel: four float4 per thread
    constexpr int kPub = kRows * (H / 4) / kThreadsU;
    auto publish = [&](const float* src, float* panel) {
        float* dst = panel + (long)g * kRows * H;
#pragma unroll
        for (int q = 0; q < kPub; ++q) {
            const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
            *reinterpret_cast<float4*>(dst + (long)r * H + 4 * c4) = *reinterpret_cast<const float4*>(src + r * HS + 4 * c4);
        }
    };

    // ---- the rows, the value normaliser, biases and the output row of weights
    const bool row_lane = tid < kRows && (long)g * kRows + tid < B;      // rows >= B: no address is formed
    if (tid < kRows) {
        int row = -1;
        long di = -1;                                      // where this row's inputs are read from
        if (row_lane) {
            const long p = u.perm[base + (long)g * kRows + tid];
            if (p >= 0 && p < u.n_rows) row = u.row_map ? u.row_map[p] : (int)p;
            di = u.pregathered ? base + (long)g * kRows + tid : row;
        }
        float rt = 0.f;
        if (di >= 0) rt = u.rtg[di];
        sRow[tid] = row;
        sRowF[tid] = 0.f; sRowF[16 + tid] = 0.f; sRowF[32 + tid] = rt;
    }
    if (tid == 64) {                                        // a lane of wave 1: the value normaliser of this mini-batch
        const int slot = (int)(mb & 1);
        float m, v;
        double cnt;
        minibatch_vn_state(u, mb, m, v, cnt);
        sMisc[2] = m; sMisc[3] = v;
        if (g == 0) { u.vn_mean[slot ^ 1] = m; u.vn_var[slot ^ 1] = v; u.vn_count[slot ^ 1] = cnt; }
    }
    for (int l = 0; l <= depth; ++l) {
        const int n = (l == depth) ? 1 : H;
        const float* bb = P + offB(l);
        for (int i = tid; i < n; i += kThreadsU) sBias[l * H + i] = bb[i];
    }
    sWout[tid] = P[offW(depth) + tid];
    for (int i = tid; i < kRows * INP; i += kThreadsU) sX[i] = 0.f;
    __syncthreads();

    // ---- gather the input rows (K4)
    {
        const float* src = u.critic_obs;
        for (int idx = tid; idx < kRows * in_dim; idx += kThreadsU) {
            const int s = idx / in_dim, i = idx - s * in_dim;
            const int row = sRow[s];
            const long di = u.pregathered ? base + (long)g * kRows + s : row;
            if (row >= 0) sX[s * INP + i] = src[di * in_dim + i];
        }
    }
    // Two fragment sets: step s of a layer uses set s & 1 (eight steps: step 0 is always set 0), and the first set of a
    // layer is requested before the barrier in front of it.
    float4 fr[2][KC];
    auto request_fwd = [&](const int l, const int step, float4 (&f)[KC]) {
        load_fwd_frags_ld<KC, true>(P + offW(l) + (step % NCH) * KW, H, (wave + kNW * (step / NCH)) * 16, lane, f);
    };
    auto request_dgrad = [&](const int l, const int step, float4 (&f)[KC]) {
        // dh[s][i] = sum_o dz[s][o] W_l[o][i]: rows o of this K chunk, columns of output tile wave + 8 (step / 2)
        load_dgrad_frags_buf_ld<KC>(P + offW(l) + (long)(step % NCH) * KW * H, H, (wave + kNW * (step / NCH)) * 16, lane, f);
    };
    if (depth > 1) request_fwd(1, 0, fr[0]);
    __syncthreads();
    {           // the block's input rows, zero padded to the panel's stride (64 .. 512 columns, a power of two): the layer-0 wgrad's K-panel
        const int xld = u.sp.xld[which], sh = __builtin_ctz((unsigned)xld);
        float* xb = u.sp.xbuf[which] + (long)g * kRows * xld;
        for (int i = tid; i < kRows * xld; i += kThreadsU) {
            const int r = i >> sh, c = i & (xld - 1);
            xb[i] = c < 16 * NT0 ? sX[r * INP + c] : 0.f;
        }
    }

    // ---- L0: first layer on MFMA, K = in_dim padded to a multiple of 16 (sX is zero padded) -> h_0 in X0
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
                bq[j] = k < in_dim ? w[k] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[k0 + 4 * j + (lane >> 4)], bq[j], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sP0[(4 * (lane >> 4) + r) * HS + o] = act_fwd(acc[r], act);
    }
    __syncthreads();

    // ---- hidden layers forward
    for (int l = 1; l < depth; ++l) {
        const float* Hp = (l & 1) ? sP0 : sP1;                // h_{l-1}
        float* Hc = (l & 1) ? sP1 : sP0;                      // h_l
        // h_{l-1}: the K-panel of dW_l, and what this workgroup reads back in the backward pass of layer l.  The stores
        // are complete (vmcnt) at the __syncthreads() that ends this layer: the workgroup-scope release every
        // __syncthreads() carries in front of its barrier.
        publish(Hp, u.sp.hbuf[which] + (long)(l - 1) * sp_plane);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < kWideSteps; ++st) {
            if (st + 1 < kWideSteps) request_fwd(l, st + 1, fr[(st + 1) & 1]);
            else if (l + 1 < depth) request_fwd(l + 1, 0, fr[0]);
            else request_dgrad(l, 0, fr[0]);                  // the first backward phase
            const int o = (wave + kNW * (st / NCH)) * 16 + (lane & 15), ch = st % NCH;
            const f32x4 part = mfma_rows_x_frags<KC>(Hp + ch * KW, HS, lane, fr[st & 1], ch ? 0.f : sBias[l * H + o]);
            if (ch == 0) acc = part; else acc += part;
            if (ch == NCH - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Hc[(4 * (lane >> 4) + r) * HS + o] = act_fwd(acc[r], act);
            }
            __builtin_amdgcn_sched_barrier(0);                // (a step's requests stay in their step: hoisted further, the sets spill)
        }
        __syncthreads();
    }
    const float* Hlast = ((depth - 1) & 1) ? sP1 : sP0;

    // ---- output layer (one output): VALU from LDS + 16-lane reductions
    if (tid < 256) {
        const int s = tid >> 4, part = tid & 15;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < HT; ++i) acc = fmaf(Hlast[s * HS + part + 16 * i], sWout[part + 16 * i], acc);
        acc = group16_sum(acc);
        if (part == 0) sOut[s * kMaxOut] = acc + sBias[depth * H];
    }
    __syncthreads();

    // ---- value loss terms of this workgroup's rows: d loss / d out -> sDOut, the rows' terms parked in sActF
    if (wave == 0)
        ppo_head_rows(u, which, 1, P, sRow, sRowF, sMisc, sActF, sOut, sDOut, lane, B);
    __syncthreads();

    // ---- output layer backward: dz_last = dOut . W_out * act'(Hlast) -> X2 (16 rows x 32 lane groups of 16 adjacent
    //      columns), and dW_out, one column per thread -- here, not at the end of the body: Hlast's plane is reused below
    {
        constexpr int CP = H / 32;
        const int s = tid >> 5, c0 = (tid & 31) * CP;
        const float d0 = sDOut[s * kMaxOut];
        float hv[CP], acc[CP], wv[CP];
        lds_read_adjacent<CP>(Hlast + s * HS + c0, hv);
        lds_read_adjacent<CP>(sWout + c0, wv);
#pragma unroll
        for (int ii = 0; ii < CP; ++ii) acc[ii] = fmaf(d0, wv[ii], 0.f) * act_bwd(hv[ii], act);
        lds_write_adjacent<CP>(sP2 + s * HS + c0, acc);
        float dw = 0.f;
#pragma unroll
        for (int r = 0; r < kRows; ++r) dw = fmaf(sDOut[r * kMaxOut], Hlast[r * HS + tid], dw);
        outrow[offW(depth) + tid] = dw;
    }
    __syncthreads();

    // ---- hidden layers backward: dgrad only (SPLIT: the weight gradients are the wgrad launch's)
    float* Dc = sP2;                                          // dz_l
    float* Dn = sP0;                                          // dz_{l-1}
    float* sHin = sP1;                                        // h_{l-1}, staged
    for (int l = depth - 1; l >= 1; --l) {
        publish(Dc, u.sp.dbuf[which] + (long)l * sp_plane);   // dz_l: the other panel of dW_l, db_l
        f32x4 acc[HT / kNW];
#pragma unroll
        for (int st = 0; st < kWideSteps; ++st) {
            if (st + 1 < kWideSteps) request_dgrad(l, st + 1, fr[(st + 1) & 1]);
            else if (l - 1 >= 1) request_dgrad(l - 1, 0, fr[0]);
            const f32x4 part = mfma_rows_x_frags<KC>(Dc + (st % NCH) * KW, HS, lane, fr[st & 1], 0.f);
            if (st % NCH == 0) acc[st / NCH] = part; else acc[st / NCH] += part;
            __builtin_amdgcn_sched_barrier(0);                // (a step's requests stay in their step: hoisted further, the sets spill)
        }
        // h_{l-1}, this workgroup's own 16 rows of the panel -> the third plane.  Requested BEHIND the layer's MFMAs: ahead
        // of them (or of the last step's), with the fragment sets in flight, the compiler parks the four float4 in scratch
        // (64 B per lane, stored and reloaded once per layer); here they cost one L2 round trip per layer beside eight
        // steps of 64 KB of weights each.  They were stored by this workgroup in the forward pass of layer l (publish
        // above) and nobody else writes them: the s_waitcnt vmcnt(0) + s_barrier of the __syncthreads() that ended that
        // layer completed the stores before any wave went on, and the waves of a workgroup share a CU and its L1, so
        // workgroup scope is enough for these loads to see them.
        float4 hin[kPub];
        {
            const float* srcp = u.sp.hbuf[which] + (long)(l - 1) * sp_plane + (long)g * kRows * H;
#pragma unroll
            for (int q = 0; q < kPub; ++q) {
                const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
                hin[q] = *reinterpret_cast<const float4*>(srcp + (long)r * H + 4 * c4);
            }
        }
#pragma unroll
        for (int q = 0; q < kPub; ++q) {
            const int i = tid + q * kThreadsU, r = i / (H / 4), c4 = i - r * (H / 4);
            *reinterpret_cast<float4*>(sHin + r * HS + 4 * c4) = hin[q];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < HT / kNW; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 4 * (lane >> 4) + r, i = (wave + kNW * t) * 16 + (lane & 15);
                Dn[s * HS + i] = acc[t][r] * act_bwd(sHin[s * HS + i], act);
            }
        }
        __syncthreads();
        float* t = Dc; Dc = Dn; Dn = t;
    }
    publish(Dc, u.sp.dbuf[which]);                            // dz_0 (its K-panel is x, published after the gather)

    // ---- what nothing inside this launch consumes: db_out (+ the segment's padding, as zeros: nothing in the workspace
    //      may be assumed to be zero), the critic's values and the block's loss partials
    if (tid >= 256 && tid < 260) {
        const int k = tid - 256;
        float acc = 0.f;
        if (k == 0) {
#pragma unroll
            for (int s = 0; s < kRows; ++s) acc += sDOut[s * kMaxOut];
        }
        outrow[offB(depth) + k] = acc;
    }
    if (wave == 6) ppo_head_values(u, sRow, sOut, lane);
    if (wave == 7) ppo_head_block(u, which, g, sMisc, sActF, lane);
}

// the critic's tiles of ppo_update_fwd_bwd_kernel<16, 32, true> (ppo_update_fwd_bwd.hpp) run the body above
template <>
__device__ __forceinline__ void ppo_update_fwd_bwd_body<kWideHT, true, true>(const UpdateDev& u, const int which, const int g) {
    (void)which;                                          // (the kernel hands a 32-tile network to its critic branch only)
    ppo_update_wide_critic_body(u, g);
}

}  // namespace ppoaf
