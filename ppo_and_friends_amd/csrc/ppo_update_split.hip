// K12, split-wgrad chain: the weight-gradient launch of its three-launch form (fwd_bwd<SPLIT> -> ppoaf_ppo_update_wgrad ->
// ppoaf_ppo_update_adam(3); the default chain ends in ONE launch instead: ppo_update_tail.hip) and the host-side layout
// queries of the split workspace (panels, the row pairs' record region).
#include "ppo_update_rowtile.hpp"
#include <hip/hip_ext.h>
#include <cstdlib>

namespace ppoaf {

// ------------------------------------------------------------------------------------------------------------
// Split-wgrad chain (the default single-rank chain): the launch between fwd_bwd<SPLIT> and Adam.  fwd_bwd's workgroups
// have published the mini-batch's inputs, hidden activations and dLoss/dz as [Bp][H] panels (u.sp); here ONE 4-wave
// workgroup forms one 16 x 16 tile of dW_l = dz_l^T . h_{l-1} over ALL B rows: every lane requests its MFMA operands
// straight from the panels (element (k, o) of dz and (k, i) of h for its k = 4 c + lane / 16: no LDS staging, all loads
// of the tile in flight at once -- the panels were written by other XCDs a moment ago, so the launch is one cold round
// trip long), wave w takes K chunks w, w + 4, ...; the four partial tiles are folded through LDS in wave order; db_l =
// the column sums of dz_l, on the tiles of input tile 0.  One workgroup per network folds the output layer's per-block
// partials in block order; the last one does the per-mini-batch bookkeeping.  Every workgroup leaves a pair of
// squared-norm partials (scaled gradients, double) for the Adam launch to add in workgroup order.  No slabs, no atomics:
// 8.7 MB of slab round trip per mini-batch at C2 become 1.6 MB of panels, and the hidden-layer wgrad MFMAs leave
// fwd_bwd's dependent chain.
// ------------------------------------------------------------------------------------------------------------
// MAXC = chunks of 16 rows a wave keeps in registers at a time (B <= 512: 32 chunks over 4 waves, one pass)
// XLD (the wide pair's launch only): the layer-0 panel's row stride is the network's u.sp.xld (64 | 128: PPOAF_SPLIT_WIDE_INPUTS;
// 256 | 512: PPOAF_SPLIT_WIDE_SHAPES); every other pair's launch keeps the constant.
// PASSES (the wide pair's launch for a mini-batch of more than 32 chunks, B > 512: PPOAF_SPLIT_WIDE_SHAPES admits B <= 1024):
// the request / MFMA sequence runs in passes of 4 MAXC = 32 chunks -- pass p covers chunks 32 p .. 32 p + 31, wave w keeps
// chunks w, w + 4, ... of them -- into the same accumulators, so a wave adds its chunks in ascending order, and parks and
// folds once.  (16 chunks per wave at once would be 192 VGPRs of operands.)  A kernel of its own (wgrad_launch): up to 32
// chunks every pair, the wide one included, runs the one-pass kernel, whose text this leaves alone.
template <int H, bool XLD, bool PASSES = false>
__device__ __forceinline__ double split_wgrad_job(const UpdateDev& u, const int which, const int job, float* sFold /* wgrad_tile.hpp */) {
    constexpr int MAXC = 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar: the chunk offsets below stay in scalar registers
    const auto& nd = u.net[which];
    const int B = (int)u.B;
    float* G = u.grads + nd.offset;
    const float sc = u.grad_scale;
    double q = 0.0;
    SplitJob sj;
    if (split_job_decode<H>(u, which, job, sj)) {
        const int ot = sj.ot, itile = sj.itile;
        const bool two = sj.two;
        // buffer loads: resource = the layer's panel, scalar offset = chunk + row quad, vector offset = the lane's constant
        // byte offset.  Rows of the last chunk beyond B are dead rows of their tile: their dz is zero and their activations
        // finite, exactly as the slab form sums them.
        const long ldx = sj.l >= 1 ? H : (XLD ? u.sp.xld[which] : 64);       // row stride of the input panel (layer 0: the gathered input rows)
        const __amdgpu_buffer_rsrc_t rd = split_panel_d<H>(u, which, sj.l), rx = split_panel_x<H>(u, which, sj.l);
        const unsigned dl = 4u * (unsigned)((lane >> 4) * H + ot * 16 + (lane & 15));
        const unsigned xl = 4u * (unsigned)((lane >> 4) * (int)ldx + itile * 16 + (lane & 15));
        const int nc = (B + 15) >> 4;                         // 16-row chunks of the mini-batch: one batch
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        float bsum = 0.f;
        {
            float a[MAXC][4], x0[MAXC][4], x1[MAXC][4];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = wave + 4 * c;
#pragma unroll
                for (int j = 0; j < 4; ++j) { a[c][j] = 0.f; x0[c][j] = 0.f; x1[c][j] = 0.f; }
                if (ch < nc) {                                // wave-uniform
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const WgradOff so = {4u * (unsigned)((16 * ch + 4 * j) * H), 4u * (unsigned)((16 * ch + 4 * j) * (int)ldx)};
                        wgrad_request_quad(rd, rx, dl, xl, xl + 64u, two, so, a[c][j], x0[c][j], x1[c][j]);
                    }
                }
            }
            wgrad_mfma<MAXC>(a, x0, x1, two, wave, nc, acc0, acc1, bsum);
        }
        if constexpr (PASSES) {
            // the same sequence again per further pass of 4 MAXC chunks, for a wave that has a chunk in it.  (A copy of the
            // block above and not a loop around it: the first pass stays textually what every other pair's kernel compiles,
            // so that those kernels keep their machine code.)
            for (int c0 = wave + 4 * MAXC; c0 < nc; c0 += 4 * MAXC) {            // c0 = the wave's first chunk of the pass (scalar)
                float a[MAXC][4], x0[MAXC][4], x1[MAXC][4];
#pragma unroll
                for (int c = 0; c < MAXC; ++c) {
                    const int ch = c0 + 4 * c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { a[c][j] = 0.f; x0[c][j] = 0.f; x1[c][j] = 0.f; }
                    if (ch < nc) {                            // wave-uniform
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const WgradOff so = {4u * (unsigned)((16 * ch + 4 * j) * H), 4u * (unsigned)((16 * ch + 4 * j) * (int)ldx)};
                            wgrad_request_quad(rd, rx, dl, xl, xl + 64u, two, so, a[c][j], x0[c][j], x1[c][j]);
                        }
                    }
                }
                wgrad_mfma<MAXC>(a, x0, x1, two, c0, nc, acc0, acc1, bsum);
            }
        }
        wgrad_park(sFold, wave, lane, acc0, acc1, bsum);
        if (wave == 0) wgrad_fold(sFold, lane, acc0, acc1);
        const long ldw = sj.ldw;
        const int i = itile * 16 + (lane & 15);               // C layout: column = lane & 15, rows 4 (lane >> 4) + r
        float bg = 0.f;
        if (wave == 0 && itile == 0 && lane < 16) bg = wgrad_bias_fold(sFold, lane);
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = ot * 16 + 4 * (lane >> 4) + r;
                if (i < ldw) { G[sj.off_w + (long)o * ldw + i] = acc0[r]; q += (double)(acc0[r] * sc) * (acc0[r] * sc); }
                if (two && i + 16 < ldw) { G[sj.off_w + (long)o * ldw + i + 16] = acc1[r]; q += (double)(acc1[r] * sc) * (acc1[r] * sc); }
            }
            if (itile == 0 && lane < 16) {
                G[sj.off_b + ot * 16 + lane] = bg;
                q += (double)(bg * sc) * (bg * sc);
            }
        }
    } else {
        // output layer (+ log_std): row-block partials -> gradient, in block order
        const long seg_off = split_off_w<H>(nd, nd.depth), seg_len = nd.size - seg_off;
        const float* outpart = u.sp.outpart[which];
        const int n_hb = (B + 15) >> 4;
        for (long idx = tid; idx < seg_len; idx += kWgradThreads) {
            const float acc = split_out_fold(outpart, n_hb, seg_len, idx);
            G[seg_off + idx] = acc;
            q += (double)(acc * sc) * (acc * sc);
        }
    }
    return q;
}

template <int HA, int HC>
__global__ __launch_bounds__(kWgradThreads) void ppo_update_wgrad_kernel(UpdateDev u, int jobs_a, int jobs_c, int per_xcd) {
    __shared__ double s_red[17];
    __shared__ __attribute__((aligned(16))) float s_fold[kWgradFoldFloats];
    const int b = blockIdx.x;
    if (b == 8 * per_xcd) { ppo_update_bookkeeping_split(u); return; }           // uniform per workgroup
    const int job = (b & 7) * per_xcd + (b >> 3);             // XCD b % 8 works on one run of the layer-major job list
    double q = 0.0;
    constexpr bool XLD = HC > 256;                            // a wide pair (PPOAF_WIDTH_PAIRS_WIDE)
    if (job < jobs_a) q = split_wgrad_job<HA, XLD>(u, 0, job, s_fold);
    else if (job < jobs_a + jobs_c) q = split_wgrad_job<HC, XLD>(u, 1, job - jobs_a, s_fold);
    const bool actor = job < jobs_a;
    q = block_sum(q, s_red);
    if (threadIdx.x == 0) {
        u.norm_scratch[6 + 2 * b] = actor ? q : 0.0;
        u.norm_scratch[7 + 2 * b] = actor ? 0.0 : q;
    }
}

// ppo_update_wgrad_kernel for a mini-batch of more than 32 chunks (the wide pair with PPOAF_SPLIT_WIDE_SHAPES, B > 512)
template <int HA, int HC>
__global__ __launch_bounds__(kWgradThreads) void ppo_update_wgrad_passes_kernel(UpdateDev u, int jobs_a, int jobs_c, int per_xcd) {
    __shared__ double s_red[17];
    __shared__ __attribute__((aligned(16))) float s_fold[kWgradFoldFloats];
    const int b = blockIdx.x;
    if (b == 8 * per_xcd) { ppo_update_bookkeeping_split(u); return; }           // uniform per workgroup
    const int job = (b & 7) * per_xcd + (b >> 3);
    double q = 0.0;
    if (job < jobs_a) q = split_wgrad_job<HA, true, true>(u, 0, job, s_fold);
    else if (job < jobs_a + jobs_c) q = split_wgrad_job<HC, true, true>(u, 1, job - jobs_a, s_fold);
    const bool actor = job < jobs_a;
    q = block_sum(q, s_red);
    if (threadIdx.x == 0) {
        u.norm_scratch[6 + 2 * b] = actor ? q : 0.0;
        u.norm_scratch[7 + 2 * b] = actor ? 0.0 : q;
    }
}

template <int HA, int HC>
static int wgrad_launch(const UpdateDev& u, hipStream_t s) {
    const int ja = split_wgrad_jobs(u.net[0]), jc = split_wgrad_jobs(u.net[1]), px = split_wgrad_per_xcd(u);
    if constexpr (HC > 256) {                                 // a wide pair (the host admits B > 512 for no other)
        if (u.B > 512) {
            hipLaunchKernelGGL((ppo_update_wgrad_passes_kernel<HA, HC>), dim3((unsigned)(8 * px + 1)), dim3(kWgradThreads), 0, s, u, ja, jc, px);
            return check_launch("ppo_update_wgrad");
        }
    }
    hipLaunchKernelGGL((ppo_update_wgrad_kernel<HA, HC>), dim3((unsigned)(8 * px + 1)), dim3(kWgradThreads), 0, s, u, ja, jc, px);
    return check_launch("ppo_update_wgrad");
}

}  // namespace ppoaf

using namespace ppoaf;

extern "C" int ppoaf_ppo_update_split_workspace_bytes(const ppoaf_ppo_update_args_t* args, int64_t* bytes_out) {
    PPOAF_REQUIRE(args && bytes_out, "ppo_update_split_workspace_bytes: null argument");
    ppoaf_ppo_update_args_t a = copy_update_args(args);
    a.split_workspace = nullptr;
    UpdateDev u;
    int rc = make_update_dev(&a, u);
    if (rc) return rc;
    // (else: update_shapes' in_dim <= 128, B <= 512, or in_dim <= 512, B <= 1024 with PPOAF_SPLIT_WIDE_SHAPES)
    if (!(args_wide_inputs(&a) && width_pair_is_wide(u.net[0].H, u.net[1].H)))
        PPOAF_REQUIRE(u.net[0].in_dim <= 64 && u.net[1].in_dim <= 64 && u.B <= 512,
                      "ppo_update_split_workspace_bytes: the split-wgrad chain covers in_dim <= 64 and B <= 512 (got %d / %d, %ld)",
                      u.net[0].in_dim, u.net[1].in_dim, u.B);
    size_t need = ws_layout(u, nullptr, nullptr);
    if (args_row_pairs(&a)) need = pair_region_offset(u) + pair_region_layout(u, nullptr, nullptr);
    *bytes_out = (int64_t)need;
    return PPOAF_OK;
}

extern "C" int ppoaf_ppo_update_row_pairs_error_offset(const ppoaf_ppo_update_args_t* args, int64_t* offset_out) {
    PPOAF_REQUIRE(args && offset_out, "ppo_update_row_pairs_error_offset: null argument");
    ppoaf_ppo_update_args_t a = copy_update_args(args);
    a.split_workspace = nullptr;
    UpdateDev u;
    int rc = make_update_dev(&a, u);
    if (rc) return rc;
    const bool pairs = args_row_pairs(&a) && pairs_run(u.net[0], u.net[1]);      // the condition of fwd_bwd's dispatch
    *offset_out = pairs ? (int64_t)pair_region_offset(u) : -1;
    return PPOAF_OK;
}

extern "C" int ppoaf_ppo_update_split_blocks(const ppoaf_ppo_update_args_t* args) {
    UpdateDev u;
    ppoaf_ppo_update_args_t a;
    if (!args) return -1;
    a = copy_update_args(args);
    a.split_workspace = nullptr;
    if (make_update_dev(&a, u)) return -1;
    return split_wgrad_blocks(u);
}

extern "C" int ppoaf_ppo_update_wgrad(const ppoaf_ppo_update_args_t* args, ppoaf_stream_t stream) {
    UpdateDev u;
    int rc = make_update_dev(args, u);
    if (rc) return rc;
    PPOAF_REQUIRE(u.split, "ppo_update_wgrad: args->split_workspace is not set (the slab chain uses ppoaf_ppo_update_reduce)");
    hipStream_t s = (hipStream_t)stream;
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) wgrad_launch<A, C>(u, s)
    PPOAF_WIDTH_PAIR_LADDER_ALL(ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("ppo_update_wgrad: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

