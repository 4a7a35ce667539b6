// What the pair forms of a one-launch GCR step share (gcr_steppair.hip step_pair_kernel, gcr_steppair_late.hip
// step_pair_late_kernel): the thread-row count, the batch sizes, the compile-time policy of the body (gcr_steppair_body.h) and the
// wave trees and the exchange of a physical workgroup that carries two logical ones.
#pragma once
#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "spmv_dev.h"
#include "exchange_dev.h"
#include "gcr_stepbuild_dev.h"

namespace mgcr {

constexpr int SP_ROWS = 2 * SB_MAX_TRIPS;   // thread-rows: u < SB_MAX_TRIPS logical workgroup A's trip u, the others B's trip u - SB_MAX_TRIPS
// Rows per batch of the pass-1 loads: 8 keeps the 128 KB of a direction per CU in flight that the keep forms have, 4 halves it —
// measured the same (298.7 / 297.2 against 298.9 / 299.6 us per cycle), 8 stays.  Rows per batch of the build and of the close pass:
// 2 (with 4 the forms at 4 and 5 directions spill, see gcr_steppair.hip).
#ifndef MGCR_SB_PAIR_P1
#define MGCR_SB_PAIR_P1 8
#endif
#ifndef MGCR_SB_PAIR_TB
#define MGCR_SB_PAIR_TB 2
#endif
// 1: the next residual r' leaves with streaming stores (st_stream) instead of plain ones, so that less of it sits dirty in the L2s
// when the launch ends.  Measured slower in every form (310.0 / 312.9 against 298.7 / 297.2 us per cycle: the next launch's gathers
// of r' lose their L2 hits): not built.
#ifndef MGCR_SB_PAIR_XR_STREAM
#define MGCR_SB_PAIR_XR_STREAM 0
#endif

// The compile-time policy of the pair body (gcr_steppair_body.h).
//   KT: thread-rows of the stored directions kept in registers from the pass-1 dots to the build, row u of Ap_j where j * 8 + u < KT:
//       the eight rows of Ap_0, then those of Ap_1, ... (the build meets them in this order).
//   LATE_R: the apply does not keep r of the thread's rows (the diagonal gather's own value is dropped); the build loads the rows
//       again from a.x, a plain load at the head of each of its batches, and holds them from there through the close pass and the
//       residual update.  Between the apply and the build nothing reads r, and its 32 registers hold kept rows instead.  The element
//       loaded is the one the gather returned — nothing writes a.x during the launch (csr_step_build asks: a.x is neither xr_out
//       nor p_out) —, so every sum keeps its operands.
//   LATE_FROM: with LATE_R, the first thread-row whose r is loaded again; the rows below keep theirs from the apply (a mixed
//       policy, for a measurement: 0 reloads all eight).
template <int KT_, bool LATE_R_, int LATE_FROM_ = 0> struct SbPairPolicy {
    static constexpr int KT = KT_, LATE_FROM = LATE_FROM_;
    static constexpr bool LATE_R = LATE_R_;
};

// The wave trees of 2 x H per-thread sums, v[0..H) logical workgroup A's and v[H..2H) B's: lds[w][(k0 + k) * 17 + wave] gets what
// block_sum_owner<NV> / sb_wave_pair_to_lds put there in a workgroup that is logical workgroup w alone.
template <int H, int LN>
__device__ __forceinline__ void sp_wave_sums_to_lds(double (&v)[2 * H], double (&lds)[2][LN], int k0) {
    static_assert(H == 1 || H == 2 || H == 4, "2 H scalars: a power of two, every lane group owns one");
    double s;
    const int k = wave_multi_sum<2 * H>(v, s);
    if (((int)threadIdx.x & (64 / (2 * H) - 1)) == 0) lds[k / H][(k0 + k % H) * 17 + ((int)threadIdx.x >> 6)] = s;
}
// ... and the waves' sums added in wave order: thread k of wave w < 2 returns logical workgroup w's total of scalar k < NV (the
// others 0.).  `lds` must not be reused before another barrier.
template <int NV, int LN>
__device__ __forceinline__ double sp_block_owner_from_lds(const double (&lds)[2][LN]) {
    __syncthreads();
    const int w = (int)threadIdx.x >> 6, k = (int)threadIdx.x & 63;
    double t = 0.;
    if (w < 2 && k < NV)
        for (int q = 0; q < RED_THREADS / 64; q++) t += lds[w][k * 17 + q];
    return t;
}

// One bounded poll of exchange_dev.h: the value of the {value, generation} slot at byte `at` once it carries `want`; gives up
// (flag in LDS, 0.) like res_collect's polls.
__device__ __forceinline__ double sp_poll(ResSync &s, int at, unsigned want) {
    int spins = 0;
    for (;;) {
        const v4i w = __builtin_amdgcn_raw_buffer_load_b128(s.slots, at, 0, RES_SC1);
        if ((unsigned)w.z == want) return __hiloint2double(w.y, w.x);
        spins++;
        if (spins > s.spin_limit || ((spins & 255) == 0 && __hip_atomic_load(s.abort_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            *s.gave_up = 1;
            return 0.;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
// res_collect (exchange_dev.h) for a physical workgroup that carries two logical ones.  The hop-1 tasks are indexed by logical
// workgroup and wave, task = wave * nblk + lb: this workgroup takes those of both its logical numbers, lbs[w & 1] on its waves w
// (as that workgroup's wave w >> 1, w >> 1 + 8, ...) — which wave folds a task does not enter its sum.  Hop 2 and the totals are
// res_collect's (the copy is logical workgroup lbs[0]'s, s.lb); the generation advances once.  Kept apart from res_collect: written as one
// function with the number of logical workgroups as a parameter, the existing kernels' instruction order changes.
template <int NVT>
__device__ __forceinline__ bool sp_collect(ResSync &s, int kind, const int (&lbs)[2]) {
    static_assert(NVT <= RES_NV, "scalars per exchange");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ng = (s.nblk + 63) >> 6;   // groups that hold workgroups
    for (int task = (wave >> 1) * s.nblk + lbs[wave & 1]; task < ng * NVT; task += (RED_THREADS / 128) * s.nblk) {   // wave-uniform
        const int g = task / NVT, k = task - g * NVT;
        const int blk = g * 64 + lane;
        const double v = blk < s.nblk ? sp_poll(s, ((kind * RES_NV + k) * RES_BLK + blk) * 16, s.gen) : 0.;
        double t = wave_sum(v);
        t = __shfl(t, 0, 64);
        if (lane < RES_COPIES) {
            const v4i w4 = {__double2loint(t), __double2hiint(t), (int)s.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, s.slots, RES_L2_BASE + ((lane * 3 + kind) * RES_NV + k) * RES_GRP * 16 + g * 16, 0, RES_SC1);
        }
    }
    if ((int)threadIdx.x < RES_GRP * NVT) {
        const int k = (int)threadIdx.x / RES_GRP, g = (int)threadIdx.x % RES_GRP;
        const int copy = s.lb & (RES_COPIES - 1);
        s.ws[k * RES_GRP + g] = g < ng ? sp_poll(s, RES_L2_BASE + ((copy * 3 + kind) * RES_NV + k) * RES_GRP * 16 + g * 16, s.gen) : 0.;
    }
    __syncthreads();
    s.gen++;
    return *s.gave_up == 0;
}

}  // namespace mgcr
