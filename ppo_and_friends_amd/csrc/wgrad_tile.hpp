// The weight-gradient tile of the split-wgrad chains (K12: ppo_update_split.hip, ppo_update_tail.hip; K14:
// icm_update.hip; K15: mat_update.hip) and the Adam step on one element that their fused forms end in.
//
// One 4-wave workgroup forms 16 output rows x 32 input columns of dW = dz^T . x over ALL rows of the mini-batch: two
// 16x16x4 f32 MFMA accumulator chains that share the dz operand, K = the rows.  Every lane requests its operands straight
// from the panels with buffer loads (resource = the panel, vector offset = the lane's constant byte offset, scalar offset
// = 16-row chunk + row quad: no vector address arithmetic per load, no LDS staging); wave w takes chunks w, w + 4, ...,
// MAXC of them in flight before the first MFMA (the panels were written by other XCDs a moment ago: a batch is one cold
// round trip).  The bias gradient is the column sum of dz.  Waves 1..3 park their partial tiles in LDS and wave 0 adds
// them in wave order:
//
//   s_fold[((w - 1) * 2 + t) * 256 + 4 * lane + r]   tile t (0 | 1) of wave w = 1..3, the lane's four C registers
//   s_fold[kWgradFoldBias + 16 * w + o]              wave w's sum of dz column o (w = 0..3), added as ((w0 + w1) + w2) + w3
//
// C layout of a tile: column = lane & 15, rows 4 (lane >> 4) + r.
#pragma once
#include "mlp_device.hpp"

namespace ppoaf {

constexpr int kWgradFoldBias = 3 * 2 * 256;                   // the parked tiles come first
constexpr int kWgradFoldFloats = kWgradFoldBias + 4 * 16;

struct WgradOff { unsigned d, x; };                           // scalar byte offsets of one row quad in the dz / x panel

__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0xFFFFFFFF, 0x00020000);
}

// The operand requests of one row quad.  two == false (uniform per workgroup): input tile 1 does not exist, x1 is left alone.
__device__ __forceinline__ void wgrad_request_quad(const __amdgpu_buffer_rsrc_t rd, const __amdgpu_buffer_rsrc_t rx, const unsigned dl,
                                                   const unsigned xl0, const unsigned xl1, const bool two, const WgradOff s, float& a, float& x0,
                                                   float& x1) {
    a = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, dl, s.d, 0));
    x0 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xl0, s.x, 0));
    if (two) x1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, xl1, s.x, 0));
}
// The MFMAs of one batch -- chunks c0, c0 + 4, ... (at most MAXC, below n_chunks; wave-uniform), four row quads each: the two
// accumulator chains and the lane's partial column sum of dz, in request order
template <int MAXC>
__device__ __forceinline__ void wgrad_mfma(const float (&a)[MAXC][4], const float (&x0)[MAXC][4], const float (&x1)[MAXC][4], const bool two,
                                           const int c0, const int n_chunks, f32x4& acc0, f32x4& acc1, float& bsum) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        if (c0 + 4 * c < n_chunks) {                          // wave-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][j], x0[c][j], acc0, 0, 0, 0);
                if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][j], x1[c][j], acc1, 0, 0, 0);
                bsum += a[c][j];
            }
        }
    }
}

// All chunks of a wave, a batch of MAXC at a time (wave-uniform trip count; both input tiles exist): every operand of a
// batch is requested before its first MFMA.  off(chunk) -> the scalar offsets of the chunk's first row quad, quad = the bytes
// from one quad to the next.  (K15.  K12 -- one batch, a run-time `two`, the tail's requests between request and use -- and
// K14 write this loop in their kernels over the same pieces: as a call it changed their register allocation or duplicated
// their loads, profiles/wgrad_tile_isa.md.)
template <int MAXC, class Off>
__device__ __forceinline__ void wgrad_accumulate(const __amdgpu_buffer_rsrc_t rd, const __amdgpu_buffer_rsrc_t rx, const unsigned dl,
                                                 const unsigned xl0, const unsigned xl1, const int wave, const int n_chunks, const Off off,
                                                 const WgradOff quad, f32x4& acc0, f32x4& acc1, float& bsum) {
    for (int c0 = wave; c0 < n_chunks; c0 += 4 * MAXC) {
        float a[MAXC][4], x0[MAXC][4], x1[MAXC][4];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ci = c0 + 4 * c;
            if (ci < n_chunks) {                              // wave-uniform
                const WgradOff s = off(ci);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    wgrad_request_quad(rd, rx, dl, xl0, xl1, true, WgradOff{s.d + j * quad.d, s.x + j * quad.x}, a[c][j], x0[c][j], x1[c][j]);
            }
        }
        wgrad_mfma<MAXC>(a, x0, x1, true, c0, n_chunks, acc0, acc1, bsum);
    }
}

// Waves 1..3 park their tiles; every wave its column sums of dz (over the lane group's rows, then over the 4 lane groups).
// Ends with the workgroup's barrier.
__device__ __forceinline__ void wgrad_park(float* s_fold, const int wave, const int lane, const f32x4 acc0, const f32x4 acc1, float bsum) {
    if (wave > 0) {
        *reinterpret_cast<f32x4*>(s_fold + (((wave - 1) * 2 + 0) * 64 + lane) * 4) = acc0;
        *reinterpret_cast<f32x4*>(s_fold + (((wave - 1) * 2 + 1) * 64 + lane) * 4) = acc1;
    }
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 16) s_fold[kWgradFoldBias + wave * 16 + lane] = bsum;
    __syncthreads();
}
// wave 0, behind wgrad_park: the parked tiles, in wave order
__device__ __forceinline__ void wgrad_fold(const float* s_fold, const int lane, f32x4& acc0, f32x4& acc1) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        acc0 += *reinterpret_cast<const f32x4*>(s_fold + ((w * 2 + 0) * 64 + lane) * 4);
        acc1 += *reinterpret_cast<const f32x4*>(s_fold + ((w * 2 + 1) * 64 + lane) * 4);
    }
}
// lanes 0..15, behind wgrad_park: the bias gradient of output row `lane` of the tile
__device__ __forceinline__ float wgrad_bias_fold(const float* s_fold, const int lane) {
    const float* s = s_fold + kWgradFoldBias + lane;
    return s[0] + s[16] + s[32] + s[48];
}

// ---- optimiser state of one bucket element and the Adam step on it (adam.hip's clip_adam_kernel, expression for
// expression; the units are built with -ffp-contract=off: the same roundings).
// BUFFER: through buffer descriptors on the three arrays, ONE 32-bit offset register per element, which stays live (the
// step's stores need the index again).  As plain global loads every request built a 64-bit address pair, the pairs were
// reused for the next element's addresses, and the compiler holds a write to the address registers of a load in flight
// back until that load has returned: the state requests waited for one another, and the first operand request for all of
// them -- a serial round trip ahead of the operands.  (4 * idx < 2^32 is the caller's to check.)  pmv_hold, behind the
// job's last request, is what keeps those offset registers from being handed to something else while the loads are in
// flight.
struct Pmv { float p, m, v; };
__device__ __forceinline__ unsigned pmv_off(const long idx) { return 4u * (unsigned)idx; }
__device__ __forceinline__ void pmv_hold(const unsigned off) { asm volatile("" :: "v"(off)); }
template <bool BUFFER>
__device__ __forceinline__ Pmv pmv_load(const float* params, const float* exp_avg, const float* exp_avg_sq, const long idx, const bool ok) {
    Pmv r = {0.f, 0.f, 0.f};
    if constexpr (!BUFFER) {
        if (ok) { r.p = params[idx]; r.m = exp_avg[idx]; r.v = exp_avg_sq[idx]; }
    } else if (ok) {
        const unsigned off = pmv_off(idx);
        r.p = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wgrad_rsrc(params), off, 0, 0));
        r.m = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wgrad_rsrc(exp_avg), off, 0, 0));
        r.v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wgrad_rsrc(exp_avg_sq), off, 0, 0));
    }
    return r;
}
// gs = grad_scale x the clip coefficient (an update that does not clip passes its grad_scale)
__device__ __forceinline__ void adam_update(Pmv& s, const float beta1, const float beta2, const float eps, const float g, const float gs,
                                            const float step_size, const float bc2_sqrt) {
    const float gi = g * gs;
    s.m = beta1 * s.m + (1.0f - beta1) * gi;
    s.v = beta2 * s.v + (1.0f - beta2) * gi * gi;
    s.p = s.p - step_size * (s.m / (sqrtf(s.v) / bc2_sqrt + eps));
}
__device__ __forceinline__ void adam_element(const float* params, float* exp_avg, float* exp_avg_sq, const float beta1, const float beta2,
                                             const float eps, const long idx, const float g, Pmv s, const float gs, const float step_size,
                                             const float bc2_sqrt) {
    adam_update(s, beta1, beta2, eps, g, gs, step_size, bc2_sqrt);
    const_cast<float*>(params)[idx] = s.p;
    exp_avg[idx] = s.m;
    exp_avg_sq[idx] = s.v;
}

}  // namespace ppoaf
