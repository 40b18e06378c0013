// What the two K14 chains share (icm_update.hip: one width H everywhere; icm_update_shapes.hip: an encoding width and
// model widths of their own): the device view of a mini-batch, the block table of the weight-gradient launch, the row
// and workgroup maps, and the host side of that launch, which lives in icm_update.hip with its kernel.
#pragma once
#include "mlp_device.hpp"

namespace ppoaf {

struct IcmDev {
    int O, H, A, Ain, d_inv, d_fwd, act, discrete;
    long enc_off, inv_off, fwd_off, enc_size, total;
    const float* params; float* grads; float* exp_avg; float* exp_avg_sq; float* slabs;
    int64_t* step_count; const float* lr;
    float beta1, beta2, adam_eps, grad_scale;
    const float* obs; const float* next_obs; const void* actions;
    const int64_t* perm; const int32_t* row_map; long n_rows;
    int64_t* cursor; long B, batch_stride, Bpad;
    float icm_beta; int fused_adam, pregathered;
    float* actE; float* dEnc; float* loss_partials; double* totals;
    int nT, confine;
    // split-wgrad chain (args->split_workspace): the three fwd_bwd kernels form NO weight gradient; they publish every
    // layer's dLoss/dz (and the inputs that are not in scratch already) as [rows][width] panels and the reduce launch
    // becomes icm_wgrad_kernel.  Panels (plane = Bpad * H floats):
    int split;
    float* xO;      // [2][Bpad][XO]   gathered observation rows of the two streams, zero padded to XO = 16 ceil(O / 16)
    float* dE;      // [2][4][plane]   encoder dz, stream-major
    float* hI;      // [d_inv][plane]  inverse model hidden activations     dI: [d_inv][plane] its dz
    float* dI;
    float* oI;      // [Bpad][16]      d(inverse model output), zero padded
    float* hF;      // [d_fwd][plane]  forward model hidden activations     dF: [d_fwd + 1][plane] its dz (last: the output layer)
    float* dF;
    float* aF;      // [Bpad][16]      the forward model's action columns (one-hot / action values), zero padded
    int XO;
};

// one [n_o x n_i] block of some weight matrix = D^T X over all rows (and both observation streams for the encoder)
struct IcmBlk {
    const float* D; const float* X;     // [rows][ldd] / [rows][ldx] panels; segment s adds s * seg_d / s * seg_x floats
    long seg_d, seg_x, w, b;            // w: bucket offset of the block's first weight; b: of its bias (-1: none from this block)
    int n_seg, ldd, ldx, n_o, n_i, ldw, job0, n_ip;
};
constexpr int kIcmMaxBlk = 16;
struct IcmWg { IcmBlk blk[kIcmMaxBlk]; int n_blk, n_jobs; int xcd_job0[9]; };   // XCD x works on jobs [xcd_job0[x], xcd_job0[x + 1])

// args->xcd_half = 1 / 2: the fwd_bwd kernels' workgroups on XCDs 0-3 / 4-7 only (workgroup b is dispatched to XCD b % 8;
// the launch is twice as wide, the other half's workgroups return at once) -> the block index the kernel works on, or -1
__device__ __forceinline__ int icm_block(const IcmDev& u) {
    const int b = blockIdx.x;
    if (!u.confine) return b;
    const int x = b & 7;
    return (x >> 2) != u.confine - 1 ? -1 : ((b >> 3) << 2) | (x & 3);
}

__device__ __forceinline__ void icm_rows(const IcmDev& u, int g, int tid, int* sRow) {
    if (tid < kRows) {
        const long s = (long)g * kRows + tid;
        int row = -1;
        if (s < u.B) {
            if (u.pregathered) {
                row = (int)(u.cursor[0] * u.batch_stride + s);   // tables in shuffled order: no index chain
            } else if (u.perm) {
                const long p = u.perm[u.cursor[0] * u.batch_stride + s];
                if (p >= 0 && p < u.n_rows) row = u.row_map ? u.row_map[p] : (int)p;
            } else {
                row = (int)s;                         // rollout-time reward: the batch is the env batch itself
            }
        }
        sRow[tid] = row;
    }
}

// host (icm_update.hip).  icm_add_block appends one block to the table; icm_deal_jobs deals the finished block-major job
// list to the 8 XCDs in runs of equal cost; icm_launch_wgrad issues icm_wgrad_kernel (+ the bookkeeping workgroup: loss ->
// totals, cursor) over the table: it reads of `u` the optimiser fields, grads, nT, B, A, H (the forward loss's mean runs over
// B x H), discrete, icm_beta, loss_partials, totals and the cursor.
void icm_add_block(IcmWg* w, const float* D, int ldd, long seg_d, const float* X, int ldx, long seg_x, int n_seg, int n_o, int n_i,
                   long wo, int ldw, long bo);
void icm_deal_jobs(IcmWg* w);
int icm_launch_wgrad(const IcmDev& u, const IcmWg& w, hipStream_t stream);
// gfx950 has 160 KB of LDS per CU; launches above the 64 KB default need the attribute set once per kernel
int allow_large_lds(const void* kernel, size_t bytes, bool& done, const char* what);

}  // namespace ppoaf
