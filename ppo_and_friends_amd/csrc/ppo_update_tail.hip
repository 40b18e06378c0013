// K12, fused tail of the split-wgrad chain (round 4): ONE launch after fwd_bwd<SPLIT> forms every weight gradient of
// the mini-batch, the two clip norms, and applies clip + Adam (ppo_policy.py:1032-1055) -- what ppoaf_ppo_update_wgrad +
// ppoaf_ppo_update_adam(compute_norms 3) did in two launches.  Per mini-batch at C2 those two launches were 10.1 us
// (5.05 + 5.01) for ~1 us of arithmetic each: a launch ramp plus a cold round trip for inputs other XCDs had just written
// (profiles/r03_update_pmc.csv: waves parked 64-72 %).  Here
//
//   * every workgroup owns one 16 x 32 piece of one layer's dW (or a network's output segment) END TO END: it requests
//     the optimiser state (p, m, v) of its elements together with its MFMA operands (one cold round trip for both),
//     forms the gradient over all B rows on MFMA (split_wgrad_job's arithmetic and fold order, bit for bit), and applies
//     Adam to exactly those elements -- the gradient never goes through memory on its way to the optimiser;
//   * the one thing every workgroup needs from every other one is the squared norm of the whole gradient (the clip
//     coefficient): each publishes its partial as ONE 16-byte record of two {32 data bits, 32-bit launch tag} granules
//     (one `sc1` store; MI355X_MICROARCH.md, data-tagged granules: no flag, no fence, no ordering needed), and one wave of
//     each workgroup polls all records with `sc1` loads until every tag is this launch's, then adds them lane-strided +
//     xor butterfly -- the association xchg_ordered_norms uses in the Adam launch, so the coefficient, and with it every
//     parameter and moment, is BITWISE what the three-launch chain produces;
//   * a bookkeeping workgroup folds the loss partials into the totals, waits for the same records, and only then
//     advances what the other workgroups read at their start (step counters, the launch tag, the mini-batch cursor).
//
// All workgroups must be resident together (C2: 153 of 256 threads on 256 CUs; 256-wide critics: 369, two to three per
// CU at this kernel's register count -- checked on the host against the occupancy the runtime reports); every wait is
// bounded by a wall-clock budget and ends in the control block's error word instead of a hang (the host then restores
// the epoch's starting state and runs the three-launch chain, fused_update.py).
#include "ppo_update_dev.hpp"
#include "tail_sync.hpp"
#include "peer_exchange_device.hpp"
#include <hip/hip_ext.h>
#include <cstddef>

namespace ppoaf {

constexpr int kTailMaxE = 9;                  // output segment: up to 9 elements per thread (8 x 256 weights + bias + log_std)

// What a job workgroup reads of the words the bookkeeping workgroup rewrites (TailPre, tail_sync.hpp): the launch tag's
// source, the network's Adam step, the learning rate and the control block's bias corrections.  The ordering contract: these words are READ (the
// load is issued and its value latched) before this workgroup publishes its record; the bookkeeping workgroup rewrites
// them only after every record carries the launch's tag, i.e. after all of these reads.
// Request and use are apart on purpose.  tail_pre_request comes right BEHIND the job's state and operand loads: a wave's
// loads retire in order, so nothing the MFMA phase waits for queues behind these words, and they have the whole MFMA and
// fold phases to land.  tail_pre_use (behind the fold, in front of wave 0's tail_publish) is where their first arithmetic
// happens -- the tag's mask and + 1, the step's + 1, the test against bc_t.  Left to itself the compiler hoists that cheap
// arithmetic up to the loads and plants a full wait with it, a cold round trip with nothing else in flight ahead of the
// first operand request (two of them, 3.7 k cycles, before this split); the empty asm is what pins the first use down.
// EVERY wave passes tail_pre_use, although only wave 0 has a use for the words: a load that some path never consumes
// stays "in flight" in the compiler's wait bookkeeping up to the end of that arm of tail_job, and the arms -- which
// exclude each other -- follow one another in the compiled text: the other arm's first write to one of those registers
// then got a `vmcnt` wait sized for THIS arm's history, which on its own history meant "everything requested so far"
// (a full round trip between the first and the second chunk of operand requests).
// The loads are relaxed atomics so that they stay where they are written: `seq` at agent scope (`sc1`, as the record
// traffic), the others at workgroup scope (plain loads, as before).
// ONE_TRIP (kTailOneTrip: both networks at most 128 wide) is the flavour that does all of this.  With a 256-wide network
// (369 workgroups at C4, two to three per CU) the same launch measured SLOWER that way in every order of requests tried
// (`<128,256>`: 10.2 - 10.9 us against 9.6), so those instantiations keep the words' loads at the start of the workgroup
// (tail_pre_load) and plain state loads, as they were.
constexpr bool kTailOneTrip(const int ha, const int hc) { return ha <= 128 && hc <= 128; }
// !ONE_TRIP: read at the START of the workgroup (`seq` by the kernel, before it branches)
__device__ __forceinline__ TailPre tail_pre_load(const UpdateDev& u, const TailDev& td, const int which, const unsigned long long seq) {
    TailPre r;
    r.seq = seq;
    r.t = (long long)u.step_counts[which];
    r.lr = u.lr[0];
    r.bc.t = td.ctl->bc_t[which];
    r.bc.bc1 = td.ctl->bc[2 * which];
    r.bc.bc2s = td.ctl->bc[2 * which + 1];
    return r;
}
__device__ __forceinline__ TailPre tail_pre_request(const UpdateDev& u, const TailDev& td, const int which) {
    TailPre r;
    r.seq = __hip_atomic_load(&td.ctl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.t = __hip_atomic_load(&u.step_counts[which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    r.lr = __hip_atomic_load(&u.lr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    r.bc.t = __hip_atomic_load(&td.ctl->bc_t[which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    r.bc.bc1 = __hip_atomic_load(&td.ctl->bc[2 * which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    r.bc.bc2s = __hip_atomic_load(&td.ctl->bc[2 * which + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return r;
}
__device__ __forceinline__ TailPre tail_pre_use(TailPre r) {
    asm volatile("" : "+v"(r.seq), "+v"(r.t), "+v"(r.lr), "+v"(r.bc.t), "+v"(r.bc.bc1), "+v"(r.bc.bc2s));
    return r;
}
// ---- N > 1: the K17 gradient exchange as a phase of the job (mpi_avg_gradients, utils/mpi_utils.py:89-111, at its call
// sites ppo_policy.py:1035,1048).  Workgroup b of every rank runs the same job, so exchange group b depends only on
// group b of its peers: the job's 16 x 32 sums (+ 16 bias sums) go to THIS rank's slot as 16-byte system-scope stores
// (slot layout = job-major tiles, private to this exchange object: [nblk][528] floats, then the two output segments),
// one lane tells every peer's flag word for (b, this rank), the peers' tiles are read back with 16-byte system-scope
// loads and added IN RANK ORDER (every rank forms the bitwise identical sum), and the job carries on with the summed
// tile: norm partial, the launch-wide wait, clip + Adam.  No fences (a system-scope acquire would drop this XCD's L2
// under the other jobs' operand panels): slot, flag and peer accesses are system-scope accesses that bypass the caches;
// a workgroup's slot stores are acknowledged (vmcnt(0) + barrier) before its flags go out, and a consumer reads a peer's
// tile only after it has seen that peer's flag.  Two slots alternate with the sequence number's parity.
constexpr int kTailTileFloats = 528;          // 16 x 32 tile + 16 bias sums
struct TailXchg { XchgDev x; long long seq, wait_ticks; long seg_base[2]; };

// xchg_sequence for a job: requested behind the job's operands, its + 1 pinned there (the same hoisting as tail_pre_use's
// words: the add would otherwise drag a full wait in front of the first operand request).  Only this workgroup's own
// thread 0 ever writes group_seq[g] (xchg_advance, at the end of the job).
__device__ __forceinline__ long long tail_xchg_sequence(const TailXchg& c, const unsigned g) {
    long long v = c.x.group_seq[g];
    asm volatile("" : "+v"(v));
    return v + 1;
}
__device__ __forceinline__ void tail_xchg_publish_wait(const TailXchg& c, const unsigned g) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const XchgDev& x = c.x;
    if (threadIdx.x == 0) {
#pragma unroll                                                // (static indices: the pointer table stays in scalar registers)
        for (int p = 0; p < kMaxPeers; ++p)
            if (p < x.n_ranks && p != x.rank)
                __hip_atomic_store(&x.peer_flags[p][g * kMaxPeers + x.rank], c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const int p = (int)threadIdx.x - 64;
    if (p >= 0 && p < x.n_ranks && p != x.rank) {
        long long budget = c.wait_ticks;
        if (__hip_atomic_load(&x.words[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) budget = 0;      // broken for good
        const long long* flag = &x.my_flags[g * kMaxPeers + p];
        const long long t0 = (long long)wall_clock64();
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < c.seq) {
            __builtin_amdgcn_s_sleep(1);
            if ((long long)wall_clock64() - t0 > budget) {
                __hip_atomic_store(&x.words[3], c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
}
// float offset `off` (a multiple of 4) inside the slot of this launch's parity: own value out, rank-ordered sum back
__device__ __forceinline__ void tail_xchg_store4(const TailXchg& c, const long off, const f32x4 v) {
    const long byte = ((c.seq & 1) * c.x.n4 * 4 + off) * 4;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(tail_u32x4, v), wgrad_rsrc(c.x.my_slots), (unsigned)byte, 0, 17 /* sc0 sc1 */);
}
__device__ __forceinline__ f32x4 tail_xchg_sum4(const TailXchg& c, const long off, const f32x4 own) {
    const long byte = ((c.seq & 1) * c.x.n4 * 4 + off) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p0 = 0; p0 < kMaxPeers; p0 += 8) {
        if (p0 >= c.x.n_ranks) break;
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = p0 + k;
            if (p >= c.x.n_ranks) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            else if (p == c.x.rank) v[k] = own;
            else v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wgrad_rsrc(c.x.peer_slots[p]), (unsigned)byte, 0, 17));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (p0 + k < c.x.n_ranks) acc += v[k];
    }
    return acc;
}
__device__ __forceinline__ void tail_xchg_store1(const TailXchg& c, const long off, const float v) {
    float* mine = reinterpret_cast<float*>(c.x.my_slots) + (c.seq & 1) * c.x.n4 * 4 + off;
    __hip_atomic_store(reinterpret_cast<unsigned*>(mine), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float tail_xchg_sum1(const TailXchg& c, const long off, const float own) {
    const long fo = (c.seq & 1) * c.x.n4 * 4 + off;
    float acc = 0.f;
#pragma unroll
    for (int p0 = 0; p0 < kMaxPeers; p0 += 8) {
        if (p0 >= c.x.n_ranks) break;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = p0 + k;
            if (p >= c.x.n_ranks) v[k] = 0.f;
            else if (p == c.x.rank) v[k] = own;
            else v[k] = __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(reinterpret_cast<const float*>(c.x.peer_slots[p]) + fo),
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (p0 + k < c.x.n_ranks) acc += v[k];
    }
    return acc;
}

// Optimiser state of bucket element idx (ONE_TRIP: through buffer descriptors, wgrad_tile.hpp; 4 * idx < 2^32 is checked on
// the host, tail_prepare) and the step on it with the coefficients tail_sync_wave0 left
struct TailCoef { float gs, step_size, bc2_sqrt; };
template <bool ONE_TRIP>
__device__ __forceinline__ Pmv tail_pmv_load(const UpdateDev& u, const long idx, const bool ok) {
    return pmv_load<ONE_TRIP>(u.params, u.exp_avg, u.exp_avg_sq, idx, ok);
}
__device__ __forceinline__ void tail_adam1(const UpdateDev& u, const long idx, const float g, const Pmv& s, const TailCoef& c) {
    adam_element(u.params, u.exp_avg, u.exp_avg_sq, u.beta1, u.beta2, u.adam_eps, idx, g, s, c.gs, c.step_size, c.bc2_sqrt);
}

// One job of the split-wgrad job list (ppo_update_split.hip: split_wgrad_job -- same tiles, same operand loads, same fold
// and summation orders), carried through to the optimiser step.  Offsets of p / m / v / G are bucket offsets.
// The 16 x 32 output tile is formed by wave 0 (C layout) and handed to ALL 256 threads through LDS for the optimiser
// step: thread t owns tile elements t and t + 256 (row e / 32, column e % 32: whole 128-byte lines of p / m / v), whose
// state it requested at the start of the job, beside the MFMA operands.
template <int H, bool XCHG, bool ONE_TRIP>
__device__ __forceinline__ void tail_job(const UpdateDev& u, const TailDev& td, const unsigned long long seq0, const int b, const int which,
                                         const int job, float* sFold /* wgrad_tile.hpp */, float* sTile /* [16][32] + [16] */,
                                         double* s_red, float* s_coef, TailXchg* xc) {
    constexpr int MAXC = 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const auto& nd = u.net[which];
    const int B = (int)u.B;
    const long nb = nd.offset;                                 // this network's first float in the bucket
    float* G = u.grads + nb;
    const float sc = u.grad_scale;
    double q = 0.0;
    TailPre pre;
    if constexpr (!ONE_TRIP) pre = tail_pre_load(u, td, which, seq0);
    TAIL_STAMP(td, 0);
    SplitJob sj;
    if (split_job_decode<H>(u, which, job, sj)) {
        const int ot = sj.ot, itile = sj.itile;
        const bool two = sj.two;
        const long ldw = sj.ldw;
        // this thread's two tile elements (and, threads 64..79 of the jobs of input piece 0, one bias): optimiser state first
        long eidx[2];
        bool eok[2];
        Pmv se[2], sb;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = tid + 256 * k, row = e >> 5, col = e & 31;
            const int i = itile * 16 + col;
            eok[k] = (col < 16 || two) && i < ldw;
            eidx[k] = nb + sj.off_w + (long)(ot * 16 + row) * ldw + i;
            se[k] = tail_pmv_load<ONE_TRIP>(u, eidx[k], eok[k]);
        }
        const bool has_b = itile == 0 && tid >= 64 && tid < 80;
        const long bidx = nb + sj.off_b + ot * 16 + (tid - 64);
        sb = tail_pmv_load<ONE_TRIP>(u, bidx, has_b);
        // buffer loads: resource = the layer's panel, scalar offset = chunk + row quad, vector offset = the lane's constant
        // byte offset.  Rows of the last chunk beyond B are dead rows of their tile: their dz is zero and their activations
        // finite, exactly as the slab form sums them.
        const long ldx = sj.l >= 1 ? H : 64;                  // row stride of the input panel (layer 0: the gathered input rows)
        const __amdgpu_buffer_rsrc_t rd = split_panel_d<H>(u, which, sj.l), rx = split_panel_x<H>(u, which, sj.l);
        const unsigned dl = 4u * (unsigned)((lane >> 4) * H + ot * 16 + (lane & 15));
        const unsigned xl = 4u * (unsigned)((lane >> 4) * (int)ldx + itile * 16 + (lane & 15));
        const int nc = (B + 15) >> 4;
        float a[MAXC][4], x0[MAXC][4], x1[MAXC][4];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = wave + 4 * c;
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[c][j] = 0.f; x0[c][j] = 0.f; x1[c][j] = 0.f; }
            if (ch < nc) {                                    // wave-uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const WgradOff so = {4u * (unsigned)((16 * ch + 4 * j) * H), 4u * (unsigned)((16 * ch + 4 * j) * (int)ldx)};
                    wgrad_request_quad(rd, rx, dl, xl, xl + 64u, two, so, a[c][j], x0[c][j], x1[c][j]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) if constexpr (ONE_TRIP) pmv_hold(pmv_off(eidx[k]));
        if constexpr (ONE_TRIP) pmv_hold(pmv_off(bidx));
        // behind the operands: the control words (read before this workgroup publishes) and the exchange's sequence number
        if constexpr (ONE_TRIP) {
            pre = tail_pre_request(u, td, which);
            if (XCHG) xc->seq = tail_xchg_sequence(*xc, (unsigned)b);
        }
        TAIL_STAMP(td, 1);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        float bsum = 0.f;
        wgrad_mfma<MAXC>(a, x0, x1, two, wave, nc, acc0, acc1, bsum);
        TAIL_STAMP(td, 2);
        wgrad_park(sFold, wave, lane, acc0, acc1, bsum);
        const int i = itile * 16 + (lane & 15);               // C layout: column = lane & 15, rows 4 (lane >> 4) + r
        float bg = 0.f;
        if (wave == 0) {
            wgrad_fold(sFold, lane, acc0, acc1);
            if (itile == 0 && lane < 16) bg = wgrad_bias_fold(sFold, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * (lane >> 4) + r;
                sTile[row * 32 + (lane & 15)] = acc0[r];
                sTile[row * 32 + 16 + (lane & 15)] = acc1[r];
            }
            if (lane < 16) sTile[512 + lane] = bg;
        }
        if (XCHG) {
            // threads 0..127: one float4 of the tile each; 128..131: the bias sums (jobs of input piece 0)
            __syncthreads();
            const bool mine = tid < 128 || (itile == 0 && tid < 132);
            const long off = (long)b * kTailTileFloats + 4 * tid;
            f32x4 own = {0.f, 0.f, 0.f, 0.f};
            if (mine) {
                own = *reinterpret_cast<const f32x4*>(sTile + 4 * tid);
                tail_xchg_store4(*xc, off, own);
            }
            tail_xchg_publish_wait(*xc, (unsigned)b);
            if (mine) *reinterpret_cast<f32x4*>(sTile + 4 * tid) = tail_xchg_sum4(*xc, off, own);
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r;
                    acc0[r] = sTile[row * 32 + (lane & 15)];
                    acc1[r] = sTile[row * 32 + 16 + (lane & 15)];
                }
                if (lane < 16) bg = sTile[512 + lane];
            }
        }
        const TailPre got = ONE_TRIP ? tail_pre_use(pre) : pre;   // every wave: see tail_pre_use
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (i < ldw) q += (double)(acc0[r] * sc) * (acc0[r] * sc);
                if (two && i + 16 < ldw) q += (double)(acc1[r] * sc) * (acc1[r] * sc);
            }
            if (itile == 0 && lane < 16) q += (double)(bg * sc) * (bg * sc);
            TAIL_STAMP(td, 3);
            // block_sum(q) of the chain's wgrad launch: only this wave contributes, and its wave sum + three zeros is exact
            q = tail_wave_sum(q);
            TAIL_STAMP(td, 4);
            tail_sync_wave0(td, b, got, u.beta1, u.beta2, u.max_norm, u.grad_scale, which, nullptr, q, s_coef);
        }
        __syncthreads();                                      // s_coef and sTile are visible
        TAIL_STAMP(td, 5);
        const TailCoef cf = {s_coef[0], s_coef[1], s_coef[2]};
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (eok[k]) tail_adam1(u, eidx[k], sTile[tid + 256 * k], se[k], cf);
        if (has_b) tail_adam1(u, bidx, sTile[512 + tid - 64], sb, cf);
        // the gradient bucket itself (nobody in this launch reads it): last, off the step's critical path
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (eok[k]) u.grads[eidx[k]] = sTile[tid + 256 * k];
        if (has_b) u.grads[bidx] = sTile[512 + tid - 64];
        TAIL_STAMP(td, 6);
    } else {
        // output layer (+ log_std): row-block partials -> gradient in block order; a thread keeps its elements
        const long seg_off = split_off_w<H>(nd, nd.depth), seg_len = nd.size - seg_off;
        const float* outpart = u.sp.outpart[which];
        const int n_hb = (B + 15) >> 4;
        Pmv se[kTailMaxE];
        float ge[kTailMaxE];
#pragma unroll
        for (int k = 0; k < kTailMaxE; ++k) {
            const long idx = tid + (long)kWgradThreads * k;
            se[k] = tail_pmv_load<ONE_TRIP>(u, nb + seg_off + idx, idx < seg_len);
            ge[k] = 0.f;
        }
        if constexpr (ONE_TRIP) {                             // behind the state loads, as in the tile jobs
            pre = tail_pre_request(u, td, which);
            if (XCHG) xc->seq = tail_xchg_sequence(*xc, (unsigned)b);
        }
#pragma unroll
        for (int k = 0; k < kTailMaxE; ++k) {
            const long idx = tid + (long)kWgradThreads * k;
            if (idx < seg_len) ge[k] = split_out_fold(outpart, n_hb, seg_len, idx);
        }
        if (XCHG) {
#pragma unroll
            for (int k = 0; k < kTailMaxE; ++k) {
                const long idx = tid + (long)kWgradThreads * k;
                if (idx < seg_len) tail_xchg_store1(*xc, xc->seg_base[which] + idx, ge[k]);
            }
            tail_xchg_publish_wait(*xc, (unsigned)b);
#pragma unroll
            for (int k = 0; k < kTailMaxE; ++k) {
                const long idx = tid + (long)kWgradThreads * k;
                if (idx < seg_len) ge[k] = tail_xchg_sum1(*xc, xc->seg_base[which] + idx, ge[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kTailMaxE; ++k) {
            const long idx = tid + (long)kWgradThreads * k;
            if (idx < seg_len) {
                G[seg_off + idx] = ge[k];
                q += (double)(ge[k] * sc) * (ge[k] * sc);
            }
        }
        // block_sum(q) in its own association (wave sums, then the wave sum of the four of them)
        q = tail_wave_sum(q);
        if (lane == 0) s_red[wave] = q;
        __syncthreads();
        const TailPre got = ONE_TRIP ? tail_pre_use(pre) : pre;   // every wave: see tail_pre_use
        if (wave == 0) {
            q = tail_wave_sum(lane < 4 ? s_red[lane] : 0.0);
            tail_sync_wave0(td, b, got, u.beta1, u.beta2, u.max_norm, u.grad_scale, which, nullptr, q, s_coef);
        }
        __syncthreads();
        const TailCoef cf = {s_coef[0], s_coef[1], s_coef[2]};
#pragma unroll
        for (int k = 0; k < kTailMaxE; ++k) {
            const long idx = tid + (long)kWgradThreads * k;
            if (idx < seg_len) tail_adam1(u, nb + seg_off + idx, ge[k], se[k], cf);
        }
    }
}

template <int HA, int HC, bool XCHG>
__global__ __launch_bounds__(kWgradThreads) void ppo_update_wgrad_adam_kernel(UpdateDev u, TailDev td, TailXchg xc) {
    __shared__ double s_red[17];
    __shared__ __attribute__((aligned(16))) float s_fold[kWgradFoldFloats];
    __shared__ float s_tile[16 * 32 + 16];
    __shared__ float s_coef[4];
    constexpr bool ONE_TRIP = kTailOneTrip(HA, HC);
    const int b = blockIdx.x;
    unsigned long long seq0 = 0;
    if constexpr (!ONE_TRIP) seq0 = __hip_atomic_load(&td.ctl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b == td.nblk) {                                       // (needs no loaded value: ONE_TRIP's job workgroups go straight to their requests)
        // bookkeeping: the totals need nobody; what other workgroups read at their start moves only after all have published
        if (threadIdx.x >= 64) return;
        const unsigned long long seq = ONE_TRIP ? __hip_atomic_load(&td.ctl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : seq0;
        const unsigned tag = tail_tag(seq);
        ppo_update_bookkeeping_totals(u);
        // while the others work: the bias corrections of the step being taken (norm_scratch, as ppo_update_bookkeeping_steps
        // leaves them) and of the NEXT step (control block: the next launch's workgroups need not compute them)
        const int w = threadIdx.x & 1;
        const long long t_now = (long long)u.step_counts[w] + 1;
        double c_now[2] = {0.0, 0.0}, c_next[2] = {0.0, 0.0};
        if (threadIdx.x < 2) {
            c_now[0] = 1.0 - pow((double)u.beta1, (double)t_now);
            c_now[1] = sqrt(1.0 - pow((double)u.beta2, (double)t_now));
            c_next[0] = 1.0 - pow((double)u.beta1, (double)(t_now + 1));
            c_next[1] = sqrt(1.0 - pow((double)u.beta2, (double)(t_now + 1)));
        }
        double sq0, sq1;
        tail_gather(td, tag, sq0, sq1);
        if (threadIdx.x < 2) {
            u.step_counts[w] = t_now;
            u.norm_scratch[2 + 2 * w] = c_now[0];
            u.norm_scratch[3 + 2 * w] = c_now[1];
            td.ctl->bc_t[w] = t_now + 1;
            td.ctl->bc[2 * w] = c_next[0];
            td.ctl->bc[2 * w + 1] = c_next[1];
        }
        if (threadIdx.x == 0) {
            __hip_atomic_store(&td.ctl->seq, seq + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (u.cursor_advance) u.cursor[0] += u.cursor_advance;
        }
        return;
    }
    const int job = (b & 7) * td.per_xcd + (b >> 3);          // XCD b % 8 works on one run of the layer-major job list
    const bool live = job < td.jobs_a + td.jobs_c;            // the same on every rank
    if (XCHG && !ONE_TRIP && live) xc.seq = xchg_sequence(xc.x, (unsigned)b);
    if (job < td.jobs_a) tail_job<HA, XCHG, ONE_TRIP>(u, td, seq0, b, 0, job, s_fold, s_tile, s_red, s_coef, &xc);   // (XCHG, ONE_TRIP: sets xc.seq)
    else if (live) tail_job<HC, XCHG, ONE_TRIP>(u, td, seq0, b, 1, job - td.jobs_a, s_fold, s_tile, s_red, s_coef, &xc);
    else if (threadIdx.x == 0)
        tail_publish(td, tail_tag(ONE_TRIP ? __hip_atomic_load(&td.ctl->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : seq0), b, 0.0);
    if (XCHG && live) xchg_advance(xc.x, xc.seq, (unsigned)b);
}

template <int HA, int HC, bool XCHG>
static int tail_launch_as(const UpdateDev& u, const TailDev& td, const TailXchg& xc, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    // every workgroup waits for every other one: all of them must fit on the device at once
    const int rc = require_all_resident(reinterpret_cast<const void*>(ppo_update_wgrad_adam_kernel<HA, HC, XCHG>), kWgradThreads,
                                        td.nblk + 1, "ppo_update_wgrad_adam");
    if (rc) return rc;
    if (e0 || e1)
        hipExtLaunchKernelGGL((ppo_update_wgrad_adam_kernel<HA, HC, XCHG>), dim3((unsigned)(td.nblk + 1)), dim3(kWgradThreads), 0, s, e0, e1, 0, u, td, xc);
    else
        hipLaunchKernelGGL((ppo_update_wgrad_adam_kernel<HA, HC, XCHG>), dim3((unsigned)(td.nblk + 1)), dim3(kWgradThreads), 0, s, u, td, xc);
    return check_launch("ppo_update_wgrad_adam");
}
template <int HA, int HC>
static int tail_launch(const UpdateDev& u, const TailDev& td, const TailXchg* xc, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (xc) return tail_launch_as<HA, HC, true>(u, td, *xc, s, e0, e1);
    return tail_launch_as<HA, HC, false>(u, td, TailXchg(), s, e0, e1);
}

static int tail_dispatch(const UpdateDev& u, const TailDev& td, const TailXchg* xc, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const int ha = u.net[0].H, hc = u.net[1].H;
#define PPOAF_WIDTH_PAIR_CALL_(A, C) tail_launch<A, C>(u, td, xc, s, e0, e1)
    PPOAF_WIDTH_PAIR_LADDER(ha, hc)
#undef PPOAF_WIDTH_PAIR_CALL_
    set_error("ppo_update_wgrad_adam: hidden widths (actor %d, critic %d) not instantiated", ha, hc);
    return PPOAF_E_INVALID;
}

static int tail_prepare(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds, UpdateDev& u, TailDev& td) {
    int rc = make_update_dev(args, u);
    if (rc) return rc;
    PPOAF_REQUIRE(u.split, "ppo_update_wgrad_adam: args->split_workspace is not set (the tail of the split-wgrad chain)");
    PPOAF_REQUIRE(ctl && (((uintptr_t)ctl) & 63) == 0, "ppo_update_wgrad_adam: control block missing or not 64-byte aligned");
    PPOAF_REQUIRE(wait_seconds > 0.0 && wait_seconds <= 600.0, "ppo_update_wgrad_adam: wait_seconds=%g", wait_seconds);
    PPOAF_REQUIRE(u.bucket_total < (1L << 30), "ppo_update_wgrad_adam: bucket of %ld floats (32-bit byte offsets: fewer than 2^30)",
                  (long)u.bucket_total);
    td.ctl = reinterpret_cast<TailCtl*>(ctl);
    td.budget = (long long)(wait_seconds * 1.0e8);
    td.jobs_a = split_wgrad_jobs(u.net[0]);
    td.jobs_c = split_wgrad_jobs(u.net[1]);
    td.per_xcd = split_wgrad_per_xcd(u);
    td.nblk = split_wgrad_blocks(u);
    PPOAF_REQUIRE(td.nblk <= 64 * kTailMaxRounds, "ppo_update_wgrad_adam: %d workgroups, a polling wave holds %d records", td.nblk,
                  64 * kTailMaxRounds);
    for (int w = 0; w < 2; ++w)
        PPOAF_REQUIRE(ws_seg_len(u.net[w]) <= (long)kWgradThreads * kTailMaxE, "ppo_update_wgrad_adam: output segment of %ld floats (at most %d)",
                      ws_seg_len(u.net[w]), kWgradThreads * kTailMaxE);
    return PPOAF_OK;
}

// floats of one exchange slot for these shapes: job-major tiles, then the two output segments (each padded to 4)
static long tail_exchange_floats(const UpdateDev& u, long* seg_base) {
    long off = (long)split_wgrad_blocks(u) * kTailTileFloats;
    for (int w = 0; w < 2; ++w) {
        if (seg_base) seg_base[w] = off;
        off += (ws_seg_len(u.net[w]) + 3) & ~3L;
    }
    return off;
}

}  // namespace ppoaf

using namespace ppoaf;

extern "C" int ppoaf_ppo_update_tail_ctl_bytes(const ppoaf_ppo_update_args_t* args, int64_t* bytes_out) {
    UpdateDev u;
    PPOAF_REQUIRE(args && bytes_out, "ppo_update_tail_ctl_bytes: null argument");
    ppoaf_ppo_update_args_t a = copy_update_args(args);
    a.split_workspace = nullptr;
    const int rc = make_update_dev(&a, u);
    if (rc) return rc;
    *bytes_out = (int64_t)kTailRecOff + 16 * (int64_t)split_wgrad_blocks(u);
    return PPOAF_OK;
}

extern "C" int ppoaf_ppo_update_tail_exchange_floats(const ppoaf_ppo_update_args_t* args, int64_t* floats_out) {
    UpdateDev u;
    PPOAF_REQUIRE(args && floats_out, "ppo_update_tail_exchange_floats: null argument");
    ppoaf_ppo_update_args_t a = copy_update_args(args);
    a.split_workspace = nullptr;
    const int rc = make_update_dev(&a, u);
    if (rc) return rc;
    *floats_out = (int64_t)tail_exchange_floats(u, nullptr);
    return PPOAF_OK;
}

extern "C" int ppoaf_ppo_update_wgrad_adam_timed(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds,
                                                 void* start_event, void* stop_event, ppoaf_stream_t stream) {
    UpdateDev u;
    TailDev td;
    int rc = tail_prepare(args, ctl, wait_seconds, u, td);
    if (rc) return rc;
    return tail_dispatch(u, td, nullptr, (hipStream_t)stream, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

extern "C" int ppoaf_ppo_update_wgrad_adam(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds, ppoaf_stream_t stream) {
    return ppoaf_ppo_update_wgrad_adam_timed(args, ctl, wait_seconds, nullptr, nullptr, stream);
}

extern "C" int ppoaf_ppo_update_wgrad_adam_exchange(const ppoaf_ppo_update_args_t* args, void* ctl, double wait_seconds,
                                                    ppoaf_peer_exchange_t* xchg, double xchg_wait_seconds, ppoaf_stream_t stream) {
    UpdateDev u;
    TailDev td;
    int rc = tail_prepare(args, ctl, wait_seconds, u, td);
    if (rc) return rc;
    PPOAF_REQUIRE(xchg && xchg->connected, "ppo_update_wgrad_adam_exchange: exchange missing or not connected");
    TailXchg xc;
    xc.x = xchg->dev;
    xc.seq = 0;
    const long need = tail_exchange_floats(u, xc.seg_base);
    PPOAF_REQUIRE(xchg->dev.n4 * 4 >= need, "ppo_update_wgrad_adam_exchange: exchange slots of %ld floats, %ld needed "
                  "(ppoaf_ppo_update_tail_exchange_floats)", (long)xchg->dev.n4 * 4, need);
    PPOAF_REQUIRE(td.nblk <= kXchgMaxGroups, "ppo_update_wgrad_adam_exchange: %d workgroups, one exchange holds %d groups", td.nblk, kXchgMaxGroups);
    PPOAF_REQUIRE(xchg->dev.n_ranks == u.n_ranks || !u.normalize_values, "ppo_update_wgrad_adam_exchange: %d ranks in the exchange, %d in args",
                  xchg->dev.n_ranks, u.n_ranks);
    PPOAF_REQUIRE(xchg_wait_seconds > 0.0 && xchg_wait_seconds <= 600.0, "ppo_update_wgrad_adam_exchange: xchg_wait_seconds=%g", xchg_wait_seconds);
    PPOAF_REQUIRE(xchg->memory_kind != 3, "ppo_update_wgrad_adam_exchange: coarse-grained exchange slots are coherent only through "
                  "fences, which this launch does not use (create the exchange with memory_kind 0, 1 or 2)");
    xc.wait_ticks = (long long)(xchg_wait_seconds * 1.0e8);
    return tail_dispatch(u, td, &xc, (hipStream_t)stream, nullptr, nullptr);
}
