// K21 at hidden width 256: one env step of a 256-wide LSTM actor / critic pair for every row of a rank in ONE launch --
// the modes (STEP, CRITIC_NEXT, INFER, MASK), the arguments and the outputs of lstm_policy_step.hip, whose entry points
// hand hidden == 256 to the two launchers below, on the split of lstm_wide.hip: tiles of 32 rows (two MFMA M tiles) per
// workgroup of 8 waves, wave w owning the hidden units [32 w, 32 w + 32) of all four gates, W_hh (1 MiB per network)
// streamed as whole 128-byte lines through the wave's two LDS slots, every fragment feeding both M tiles.
//
// The recurrence, LayerNorm and feed-forward head are K18's 256-wide forward in its step form
// (lstm_wide_device.hpp: lstm_wide_rows_forward<true, XRows>): one step, the first W_hh tile requested ahead of the x / h
// / c loads, the last Linear's rows left in LDS.  The heads then run one lane per row (tid < 32) on K6's / K19's
// functions (action_heads.hpp) with the global row number, so the Philox counter of row e is offset + e as at every
// other width.  The networks' (h, c) are stepped IN PLACE: a workgroup reads only its own 32 rows, all before its first
// barrier, and writes them after the cell.  The sums are K18's in K18's order: the stepped states are bitwise those of
// ppoaf_lstm_forward at S = 1.
//
// STEP runs 8 * ceil(n_wg / 4) workgroups for n_wg = ceil(E / 32) row tiles, XCD-grouped as at the other widths: blocks
// 0-3 mod 8 are the actor's, 4-7 the critic's, so the eight XCDs that take consecutive workgroups split into four that
// stream the actor's W_hh and four the critic's.  CRITIC_NEXT and INFER run one workgroup per tile.  MASK, the zeroing
// alone, is a small kernel without the forward's LDS.  The block form (STEP and CRITIC_NEXT) reads the observations
// through the table of row blocks and writes the env's action blocks; it instantiates the same body with the same row
// numbers, so for equal inputs both forms store equal bits.
#include "action_heads.hpp"
#include "lstm_step_device.hpp"
#include "lstm_wide_device.hpp"

namespace ppoaf {
namespace {

extern __shared__ __attribute__((aligned(16))) unsigned char lstm_wide_step_smem[];

// the four stored rows of the tile's envs that terminated at this step: zero.  `per`: 0 -- one byte per row; else the
// block form's rule, the env's byte (row n % per of a block) serves each of its agents' rows
__device__ __forceinline__ void wide_zero_terminated(const LstmStepDev& u, const long e0, const unsigned per, const int nt) {
    for (int i = threadIdx.x; i < kWRows * kWH; i += nt) {
        const int r = i / kWH;
        const long n = e0 + r;
        if (n < u.E && u.terminated[per ? (unsigned)n % per : (unsigned)n]) {
            const long at = n * kWH + (i - r * kWH);
#pragma unroll
            for (int q = 0; q < 4; ++q) u.stored[q][at] = 0.f;
        }
    }
}

// One workgroup of a STEP, CRITIC_NEXT or INFER launch.  BLOCKS: tb is the block table (else it is not read).
template <bool BLOCKS>
__device__ __forceinline__ void wide_step_tile(const LstmStepDev& u, const LstmStepBlocks* tb) {
    const int tid = threadIdx.x;
    int which, g;
    if (u.mode == PPOAF_LSTM_STEP) {
        const int b = blockIdx.x;
        which = (b >> 2) & 1;
        g = ((b >> 3) << 2) | (b & 3);
    } else {
        which = u.mode == PPOAF_LSTM_INFER ? 0 : 1;
        g = blockIdx.x;
    }
    if (g >= u.n_wg) return;
    const long e0 = (long)g * kWRows;
    const LstmArgs& a = u.net[which];
    float* lds = reinterpret_cast<float*>(lstm_wide_step_smem);
    float* oc = which == 0 ? u.obs_out : u.critic_obs_out;
    // the forward first (its weight request leads the kernel), the observation copies into buffer row t behind it
    const float* sOut;
    if constexpr (BLOCKS) {
        const LstmXBlocks xr{which == 0 ? tb->obs : tb->critic_obs, tb->rows_per_block};
        sOut = lstm_wide_rows_forward<true, LstmXBlocks>(a, g, lds, xr);
        if (oc) {
            const int I = a.I;
            for (int i = tid; i < kWRows * I; i += kWThreads) {
                const int r = i / I, k = i - r * I;
                if (e0 + r < u.E) oc[(e0 + r) * I + k] = xr.row(e0 + r, I)[k];
            }
        }
    } else {
        sOut = lstm_wide_rows_forward<true>(a, g, lds);
        if (oc) {
            const long lo = e0 * a.I, hi = (e0 + kWRows < u.E ? e0 + kWRows : u.E) * a.I;
            for (long i = lo + tid; i < hi; i += kWThreads) oc[i] = a.x[i];
        }
    }

    // heads: one lane per env row
    if (tid < kWRows && e0 + tid < u.E) {
        const float* zr = sOut + tid * kLFS;
        const long e = e0 + tid;
        if (which == 1) {
            float v = zr[0];
            if (u.normalize_values) v = u.vn_mean[0] + v * sqrtf(u.vn_var[0] + 1e-8f);   // misc.py:124-128
            u.value_out[e] = v;
        } else if (u.mode == PPOAF_LSTM_INFER) {
            const bool greedy = u.infer_mode == PPOAF_INFER_DETERMINISTIC;
            if (u.head_kind == PPOAF_HEAD_CATEGORICAL)
                cat_infer_row(zr, a.O, greedy, e, u.seed, u.offset, u.action_out);
            else
                gauss_infer_row(zr, a.O, greedy, u.log_std, u.min_std, u.act_lo, u.act_hi, e, u.seed, u.offset, u.action_out);
        } else {
            if (u.head_kind == PPOAF_HEAD_CATEGORICAL)
                cat_step_row(zr, a.O, u.forced_raw_action, e, u.seed, u.offset, u.raw_action_out, u.action_out, u.logp_out);
            else
                gauss_step_row(zr, a.O, u.log_std, u.min_std, u.act_lo, u.act_hi, u.forced_raw_action, e, u.seed, u.offset,
                               u.raw_action_out, u.action_out, u.logp_out);
            if constexpr (BLOCKS) {
                // the row's env action, as this lane stored it in the buffer row, also into the env's action tensor
                const unsigned b = (unsigned)e / tb->rows_per_block;
                const long r = (long)((unsigned)e - b * tb->rows_per_block);
                if (u.head_kind == PPOAF_HEAD_CATEGORICAL) {
                    reinterpret_cast<int64_t*>(tb->env_action[b])[r] = reinterpret_cast<const int64_t*>(u.action_out)[e];
                } else {
                    const int n = tb->action_elems;
                    const float* src = reinterpret_cast<const float*>(u.action_out) + e * n;
                    float* dst = reinterpret_cast<float*>(tb->env_action[b]) + r * n;
                    for (int k = 0; k < n; ++k) dst[k] = src[k];
                }
            }
        }
    }

    // CRITIC_NEXT: the rows the step stored for the envs that terminated at it are zeroed
    if (u.terminated && u.mode == PPOAF_LSTM_CRITIC_NEXT)
        wide_zero_terminated(u, e0, BLOCKS ? tb->rows_per_block : 0u, kWThreads);
}

__global__ __launch_bounds__(kWThreads) void lstm_wide_step_kernel(const LstmStepDev u) {
    wide_step_tile<false>(u, nullptr);
}

__global__ __launch_bounds__(kWThreads) void lstm_wide_step_blocks_kernel(const LstmStepDev u, const LstmStepBlocks tb) {
    wide_step_tile<true>(u, &tb);
}

constexpr int kWMaskThreads = 256;
__global__ __launch_bounds__(kWMaskThreads) void lstm_wide_mask_kernel(const LstmStepDev u) {
    if ((int)blockIdx.x < u.n_wg && u.terminated) wide_zero_terminated(u, (long)blockIdx.x * kWRows, 0u, kWMaskThreads);
}

unsigned grid_of(const LstmStepDev& u) {
    return u.mode == PPOAF_LSTM_STEP ? 8u * (unsigned)((u.n_wg + 3) / 4) : (unsigned)u.n_wg;
}

}  // namespace

int lstm_wide_step(const LstmStepDev& u, hipStream_t stream) {
    if (u.mode == PPOAF_LSTM_MASK) {
        hipLaunchKernelGGL(lstm_wide_mask_kernel, dim3((unsigned)u.n_wg), dim3(kWMaskThreads), 0, stream, u);
        return check_launch("lstm_policy_step");
    }
    static bool raised = false;
    constexpr size_t lds = kWFwdLds * sizeof(float);
    if (int rc = allow_large_lds(lstm_wide_step_kernel, lds, raised, "lstm_policy_step")) return rc;
    hipLaunchKernelGGL(lstm_wide_step_kernel, dim3(grid_of(u)), dim3(kWThreads), lds, stream, u);
    return check_launch("lstm_policy_step");
}

int lstm_wide_step_blocks(const LstmStepDev& u, const LstmStepBlocks& tb, hipStream_t stream) {
    static bool raised = false;
    constexpr size_t lds = kWFwdLds * sizeof(float);
    if (int rc = allow_large_lds(lstm_wide_step_blocks_kernel, lds, raised, "lstm_policy_step_blocks")) return rc;
    hipLaunchKernelGGL(lstm_wide_step_blocks_kernel, dim3(grid_of(u)), dim3(kWThreads), lds, stream, u, tb);
    return check_launch("lstm_policy_step_blocks");
}

}  // namespace ppoaf
