// What the one-launch GCR step kernels of gcr_stepbuild.hip (two logical workgroups per CU, one each per physical workgroup) and of
// gcr_steppair.hip (one physical workgroup per CU that carries two logical ones) share: the argument block, the scalar stage's
// staged operands and the reductions that become final a pair of sums at a time.  Device side, gfx950.
#pragma once
#include <type_traits>

#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "exchange_dev.h"

namespace mgcr {

constexpr int SB_MAX_TRIPS = 4;     // rows per thread whose Ar stays in LDS (4 x 1024 x 16 B = 64 KB per workgroup)
constexpr int SB_MAX_ND = 5;

struct StepBuildArgs {
    RowMat m;
    const cplx *x;           // the residual the step applies the operator to (= the direction's start D_k)
    const cplx *aps[SB_MAX_ND];
    int64_t n;
    int nlogical;
    RowMap rm;
    DevState *st;
    int it;
    const double *partsR;    // |r|^2 partials of the residual update that ran before
    int nblkR, strideR;
    double *hist;
    int hist_cap;
    const cplx *den;
    cplx *ap_out;
    double *partsA;
    LeanCoef *lc;
    // CLOSE: the step that closes a restart cycle (gcr.hip build_close_kernel): the cycle's directions, its first one rewritten, x updated
    const cplx *ps[SB_MAX_ND];
    cplx *p_out;
    cplx *xvec;
    // XR: the NEXT step's residual update (gcr.hip xr_update_kernel<true, true>) at the end of this launch
    cplx *xr_out;            // where it leaves r - alpha Ap' (the next ring slot)
    cplx *xr_den_slot;
    int xr_slot;
    double *partsR_out;
    v4i *slots;
    unsigned gen0;
    unsigned *abort_dev;
    int *abort_host;
    int spin_limit;
    int test_stall;          // tests: logical workgroup test_stall - 1 leaves before publishing anything (0: nobody)
};

// The scalar part of a residual update (gcr.hip xr_update_kernel<true, true>) behind its exchange: alpha = <r,Ap'> / <Ap',Ap'>
// in scalar registers; logical workgroup 0 records the denominator and the pending x update.
__device__ __forceinline__ cplx sb_xr_alpha(const ResSync &sy, DevState *st, LeanCoef *lc, cplx *xr_den_slot, int xr_slot, int lb) {
    const cplx num = make_double2(res_total(sy, 0), res_total(sy, 1)), den = make_double2(res_total(sy, 2), res_total(sy, 3));
    const cplx alpha = to_sgpr(cdiv(num, den));
    if (lb == 0 && threadIdx.x == 0) {
        *xr_den_slot = den;
        st->npend = xr_slot + 1;
    }
    if (lb == 0 && (int)threadIdx.x < LND) lean_pending_update(lc, xr_slot, alpha, (int)threadIdx.x);
    return alpha;
}

// p + off bytes, with p a wave-uniform (scalar) address and off a 32-bit byte offset: the load or store takes the saddr form
template <class T>
__device__ __forceinline__ T *sb_elem(T *p, uint32_t off) {
    using C = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T *>(reinterpret_cast<C *>(p) + off);
}

// block_sum_owner<NV> (reduce.h) in two halves, for per-thread sums that become final a pair at a time: each pair goes through
// the wave trees as soon as it is final — wave_multi_sum sums every scalar by the same tree whatever NV is (same operands,
// same order: reduce.h), so lds[k * 17 + wave] holds the bits block_sum_owner<NV> puts there — and the waves' sums are
// added in wave order once all pairs are in.  `lds` must not be reused before another barrier.
__device__ __forceinline__ void sb_wave_pair_to_lds(double (&v)[2], double *lds, int k0) {
    double s;
    const int k = wave_multi_sum<2>(v, s);
    if (((int)threadIdx.x & 31) == 0) lds[(k0 + k) * 17 + ((int)threadIdx.x >> 6)] = s;
}
template <int NV>
__device__ __forceinline__ double sb_block_owner_from_lds(double *lds) {
    const int nwave = (blockDim.x + 63) >> 6;
    __syncthreads();
    double t = 0.;
    if (threadIdx.x < NV)
        for (int w = 0; w < nwave; w++) t += lds[threadIdx.x * 17 + w];
    return t;
}

// The keep body's scalar stage in two halves (gcr_stepbuild_keep_body.h: its operands are fetched behind the apply).
// Slot i of the staged operands: den[i] | lc->cx[i - nd] | entry j of column m of the coefficient table, i - 2 nd = m nd + j — the
// operand lean_close_coef multiplies beta_j by for cp_m (j > m; the other entries of the square are loaded and never used:
// they lie inside the table).
template <int NDT>
__device__ __forceinline__ const cplx *sb_stage_src(const cplx *den, const LeanCoef *lc, int i) {
    if (i < NDT) return den + i;
    if (i < 2 * NDT) return lc->cx + (i - NDT);
    const int m = (i - 2 * NDT) / NDT, j = (i - 2 * NDT) % NDT;
    return m == 0 ? lc->t + j : lc->T + j * LND + m;
}
// lean_close_coef (gcr_dev.h) on such a column: the same operands in the same order
template <int NDT>
__device__ __forceinline__ cplx sb_stage_close_coef(const cplx *col, const cplx *sbeta, int m) {
    cplx c = make_double2(0., 0.);
    for (int j = m; j < NDT; j++) c = cadd(c, cmul(sbeta[j], j == m ? make_double2(1., 0.) : col[j]));
    return c;
}
// fold_partials<1> (reduce.h) in two halves.  First: v = the thread's partial (0. beyond nblk), every wave's tree, lane 0 stores
// its wave's sum; nblk == 1 (a value that is already folded): thread 0 holds parts[0] + 0. and parks it.  Behind a barrier, any
// thread: the waves' sums added in wave order from 0. — block_sum_bcast's total, which it then hands to every thread.
__device__ __forceinline__ void sb_stage_rr_waves(double v, int nblk, double *lds_rr) {
    if (nblk == 1) {
        if (threadIdx.x == 0) lds_rr[16] = v;
        return;
    }
    double w[1] = {v}, s;
    wave_multi_sum<1>(w, s);
    if ((threadIdx.x & 63) == 0) lds_rr[threadIdx.x >> 6] = s;
}
__device__ __forceinline__ double sb_stage_rr(int nblk, const double *lds_rr) {
    if (nblk == 1) return lds_rr[16];
    const int nwave = (blockDim.x + 63) >> 6;
    double t = 0.;
    for (int w = 0; w < nwave; w++) t += lds_rr[w];
    return t;
}

// gcr_steppair.hip: the pair form of a keep step (nullptr: that step has none in this build / by the gate), its dynamic LDS, its grid
const void *sb_pair_kernel(int nd, bool xr, bool close, bool realc);
// gcr_steppair_late.hip: its late-r form (nullptr: none built / not by the gate and option step_build_pair_late / pair forms off)
const void *sb_pair_late_kernel(int nd, bool xr, bool close, bool realc);
constexpr size_t SB_PAIR_LDS = sizeof(cplx) * RED_THREADS * 2 * SB_MAX_TRIPS;   // A r of eight rows per thread
constexpr int SB_PAIR_LOGICAL = 512, SB_PAIR_GRID = SB_PAIR_LOGICAL / 2;

}  // namespace mgcr
