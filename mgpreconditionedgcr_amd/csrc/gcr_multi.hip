// Batched restarted GCR: k independent systems A x_j = b_j advance in lockstep and share every launch.
//
// The recurrences are those of the LEAN restart cycle of the single solve (gcr.hip: xr_update_kernel<true, true>,
// multidot_kernel, build_lean_kernel, close_x_kernel + build_lean_kernel(closing), flush_x_kernel), carried out per column:
//   * the work vectors (r, A r, the residual ring / P0 and the Ap slots) are multi-vectors in the interleaved layout;
//   * every column has its own device-resident state — MState::st[j] (a DevState: stop flag, iteration count, |b|^2, |r|^2),
//     its coefficient table lc[j], its cached <Ap_i, Ap_i> and its alpha / beta / closing coefficients.  A column whose
//     state has stopped is FROZEN: every kernel masks its stores to that column, so its x, r and history stay what they were
//     at its last step while the other columns go on;
//   * per step: one scalar kernel (alpha), the residual update, the k-wide apply (spmm.hip), the k-wide beta dots, one scalar
//     kernel (betas, step bookkeeping, coefficient table), the k-wide build — the scalar kernels run one workgroup per
//     column and fold the partial slabs with fold_partials, as the single kernels do in their prologues.
// Rule for the arithmetic: rows per thread, grid size, summation trees and folds are those of the single kernels (multi_dev.h),
// the element-wise expressions are copied from them: history, iteration count, convergence flag and x of column j are
// bit-identical to mgcr_gcr_solve on (A, param, rhs_j) wherever that solve sums in the plain row order (see include/mgcr.h).
//
// With a flexible right preconditioner M (gcr_multi_run only; host code — MRun::precondition — on the kernels above): the single lean
// cycle's flexible form per column, r in place in MWork::r, D = M r in the slot of the next direction or in MWork::z on a closing
// step.  M is a low-precision GCR, run as the k-wide lockstep inner solve of gcr32_multi.hip, or any operator of the k-wide apply; the
// kernels that keep it off the frozen columns' slots are gcr_multi_flex.hip's (Rule F of include/mgcr.h).
#include <climits>
#include <cmath>

#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "multi_dev.h"
#include "queue_plan.h"   // host only: the schedule of the queued solve

namespace mgcr {

struct MCoef {   // per column: this step's coefficients, written by the scalar kernels, read by the streaming ones
    cplx alpha[MV_MAX_K];
    cplx beta[MV_MAX_K][LND];
    cplx cp[MV_MAX_K][LND];   // closing step: P0' = dir - sum_m cp_m (P0, D_1 ...)
};
struct MPtrs {   // slots of a restart cycle: ps[0] = P0, ps[m] = D_m; aps[j] = A p_j
    const cplx *ps[LND];
    const cplx *aps[LND];
};

__device__ __forceinline__ bool m_active(const DevState *st, int col, int k, int it) {
    return col < k && !(st[col].stop_at < st[col].base + it);
}

// QUEUED: the kernel serves the queued solve (gcr_queue_run), true, or the batched one (gcr_multi_run), false.  The queued solve
// admits columns at different steps, so a column's LAST step (own step number == max_it) is not the launch's: such a column takes the
// finishing bookkeeping (m_finish_kernel<true>, which freezes it with stop_at == its step number) while its neighbours run a full
// step, and the kernels behind that bookkeeping — coefficients, closing x update, build — must leave it alone although
// stop_at == base + it reads as active.  That test is all QUEUED changes in them, so both solves run ONE body and the bit-for-bit
// rule needs no second copy.  The flag sits on the __global__ function itself (max_it is read by the QUEUED forms only): each
// instantiation then compiles to the code of a kernel written out for it, whereas a body shared through an inlined __device__
// function compiles to other code for the batched entries (the work-group size is then looked up, not assumed).
template <bool QUEUED>
__device__ __forceinline__ bool col_active(const DevState *st, int col, int k, int it, int max_it) {
    if constexpr (QUEUED) return m_active(st, col, k, it) && st[col].base + it < max_it;
    else return m_active(st, col, k, it);
}

struct QFields {   // queued solve, per column: the system's Fields (by value in the kernel arguments)
    const cplx *b[MV_MAX_K];
    cplx *x[MV_MAX_K];
};

__global__ void m_reset_kernel(DevState *st, double tol2, int k) {
    const int j = threadIdx.x;
    if (j >= MV_MAX_K) return;
    st[j].stop_at = j < k ? INT_MAX : -1;
    st[j].base = 0;
    st[j].iter = 0;
    st[j].npend = 0;
    st[j].bnorm2 = 0.;
    st[j].rr = 0.;
    st[j].tol2 = tol2;
    st[j].closed = 0;
}

// |b|^2, |r|^2, <r,Ap>, <Ap,Ap> per column in one pass (norm_partials_kernel, norm_partials_kernel, dot2_partials_kernel).
// QUEUED: pass 2 of an admission point (`mask`: bit j = column j is admitted).  Only the admitted columns take part — a continuing
// column's sums (the closing step's build wrote them) stay — and ap, which the k-wide apply left in the `ar` block, goes into
// slot 0 (ap0) of the admitted columns on the way.
template <int KC, bool QUEUED>
__global__ void __launch_bounds__(RED_THREADS) m_init_partials_kernel(const cplx *__restrict__ b, const cplx *__restrict__ r,
                                                                      const cplx *__restrict__ ap, int64_t n, int k, double *__restrict__ partsN,
                                                                      double *__restrict__ partsR, double *__restrict__ partsA, unsigned mask,
                                                                      cplx *__restrict__ ap0) {
    __shared__ double lds[6 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    if constexpr (QUEUED)
        if (((mask >> c0) & ((1u << KC) - 1u)) == 0) return;   // (uniform over the workgroup)
    double v[6 * KC];
#pragma unroll
    for (int s = 0; s < 6 * KC; s++) v[s] = 0.;
    MV_GRID_STRIDE(i, n) {
        cplx bv[KC], rv[KC], av[KC];
        mv_load<KC>(b, i, k, c0, bv);
        mv_load<KC>(r, i, k, c0, rv);
        mv_load<KC>(ap, i, k, c0, av);
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if constexpr (QUEUED)
                if (c0 + c < k && ((mask >> (c0 + c)) & 1u)) ap0[i * k + c0 + c] = av[c];
            v[6 * c + 4] += bv[c].x * bv[c].x + bv[c].y * bv[c].y;
            v[6 * c + 5] += rv[c].x * rv[c].x + rv[c].y * rv[c].y;
            const cplx t = cconj_mul(rv[c], av[c]);
            v[6 * c] += t.x; v[6 * c + 1] += t.y;
            const cplx u = cconj_mul(av[c], av[c]);
            v[6 * c + 2] += u.x; v[6 * c + 3] += u.y;
        }
    }
    const double tot = block_sum_owner<6 * KC>(v, lds);
    const int t = (int)threadIdx.x;
    if (t < 6 * KC) {
        const int col = c0 + t / 6, s = t % 6;
        if (col < k && (!QUEUED || ((mask >> col) & 1u))) {
            if (s < 4) partsA[(size_t)(col * 4 + s) * RED_MAX_BLOCKS + blockIdx.x] = tot;
            else if (s == 4) partsN[(size_t)col * RED_MAX_BLOCKS + blockIdx.x] = tot;
            else partsR[(size_t)col * RED_MAX_BLOCKS + blockIdx.x] = tot;
        }
    }
}

// step 0 bookkeeping (init_kernel), one workgroup per column
__global__ void __launch_bounds__(RED_THREADS) m_init_kernel(DevState *st, const double *__restrict__ partsN, const double *__restrict__ partsR,
                                                             int nblk, double *__restrict__ hist, int hist_cap) {
    __shared__ double lds[17];
    const int j = blockIdx.x;
    if (st[j].stop_at < 0) return;
    double b[1], r[1];
    fold_partials<1>(partsN + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, b, lds);
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, r, lds);
    if (threadIdx.x == 0) {
        st[j].bnorm2 = b[0];
        st[j].rr = r[0];
        hist[(size_t)j * hist_cap] = sqrt(r[0]) / sqrt(b[0]);
    }
}

// alpha = <r,Ap>/<Ap,Ap> and the pending-x bookkeeping of xr_update_kernel<true, true>'s prologue, one workgroup per column
__global__ void __launch_bounds__(RED_THREADS) m_alpha_kernel(DevState *st, int it, const double *__restrict__ partsA, int nblk, cplx *__restrict__ den,
                                                              int slot, LeanCoef *__restrict__ lc, MCoef *__restrict__ coef) {
    __shared__ double lds[4 * 17];
    const int j = blockIdx.x;
    if (st[j].stop_at < st[j].base + it) return;
    double s[4];
    fold_partials<4>(partsA + (size_t)j * 4 * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, s, lds);
    const cplx num = make_double2(s[0], s[1]), dn = make_double2(s[2], s[3]);
    const cplx alpha = cdiv(num, dn);
    if (threadIdx.x == 0) {
        den[j * LND + slot] = dn;
        st[j].npend = slot + 1;
        coef->alpha[j] = alpha;
    }
    if ((int)threadIdx.x < LND) lean_pending_update(lc + j, slot, alpha, (int)threadIdx.x);
}

// r' = r - alpha Ap into the residual ring, |r'|^2 partials (the loop of xr_update_kernel<true, true>)
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) m_xr_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef, const cplx *ap,
                                                           const cplx *r_in, cplx *r_out, int64_t n, int k, double *__restrict__ partsR) {
    __shared__ double lds[KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    cplx alpha[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = m_active(st, c0 + c, k, it);
        alpha[c] = act[c] ? coef->alpha[c0 + c] : make_double2(0., 0.);
        any = any || act[c];
    }
    if (!any) return;   // (uniform over the workgroup)
    double v[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) v[c] = 0.;
    MV_GRID_STRIDE(i, n) {
        cplx rv[KC], av[KC];
        mv_load<KC>(r_in, i, k, c0, rv);
        mv_load<KC>(ap, i, k, c0, av);
#pragma unroll
        for (int c = 0; c < KC; c++) {
            const cplx rn = csub(rv[c], cmul(alpha[c], av[c]));
            if (act[c]) r_out[i * k + c0 + c] = rn;
            v[c] += rn.x * rn.x + rn.y * rn.y;
        }
    }
    const double tot = block_sum_owner<KC>(v, lds);
    const int t = (int)threadIdx.x;
    if (t < KC && m_active(st, c0 + t, k, it)) partsR[(size_t)(c0 + t) * RED_MAX_BLOCKS + blockIdx.x] = tot;
}

// the last step a solve can run: bookkeeping only (finish_step_kernel).  QUEUED: for the columns at their OWN last step, which are
// then frozen
template <bool QUEUED>
__global__ void __launch_bounds__(RED_THREADS) m_finish_kernel(DevState *st, int it, const double *__restrict__ partsR, int nblk,
                                                               double *__restrict__ hist, int hist_cap, int max_it) {
    __shared__ double lds[17];
    const int j = blockIdx.x;
    if (st[j].stop_at < st[j].base + it) return;
    if constexpr (QUEUED)
        if (st[j].base + it != max_it) return;
    double rr[1];
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, rr, lds);
    if (threadIdx.x == 0) {
        close_step(st + j, it, rr[0], hist + (size_t)j * hist_cap, hist_cap, false);
        if constexpr (QUEUED) st[j].stop_at = st[j].base + it;
    }
}

// <Ar, Ap_d> (conj on Ar) for the NDT directions of chunk blockIdx.z and the KC columns of group blockIdx.y; rows dealt by the
// RowMap of multidot_kernel / the fused apply kernels -> partsB[((col * LND + d) * 2 + {0, 1})][blk]
template <int KC, int NDT>
__global__ void __launch_bounds__(RED_THREADS) m_dot_kernel(const cplx *__restrict__ ar, MPtrs d, int lim, int64_t n, int k, RowMap rm,
                                                            double *__restrict__ partsB) {
    __shared__ double lds[2 * KC * NDT * 17];
    const int c0 = (int)blockIdx.y * KC, d0 = (int)blockIdx.z * NDT;
    double v[2 * KC * NDT];
#pragma unroll
    for (int s = 0; s < 2 * KC * NDT; s++) v[s] = 0.;
    const cplx *dp[NDT];
#pragma unroll
    for (int q = 0; q < NDT; q++) dp[q] = d.aps[d0 + q < lim ? d0 + q : 0];
    int64_t first, end, step;
    row_range(rm, (int)blockIdx.x, (int)gridDim.x, n, &first, &end, &step);
    for (int64_t i = first; i < end; i += step) {
        cplx a[KC], b[NDT][KC];
        mv_load<KC>(ar, i, k, c0, a);
#pragma unroll
        for (int q = 0; q < NDT; q++) mv_load<KC>(dp[q], i, k, c0, b[q]);
#pragma unroll
        for (int c = 0; c < KC; c++)
#pragma unroll
            for (int q = 0; q < NDT; q++) {
                const cplx t = cconj_mul(a[c], b[q][c]);
                v[2 * (c * NDT + q)] += t.x;
                v[2 * (c * NDT + q) + 1] += t.y;
            }
    }
    const double tot = block_sum_owner<2 * KC * NDT>(v, lds);
    const int t = (int)threadIdx.x;
    if (t < 2 * KC * NDT) {
        const int col = c0 + t / (2 * NDT), q = (t / 2) % NDT;
        if (col < k && d0 + q < lim) partsB[(size_t)((col * LND + d0 + q) * 2 + (t & 1)) * RED_MAX_BLOCKS + blockIdx.x] = tot;
    }
}

// the prologue of build_lean_kernel / build_close_kernel, one workgroup per column: betas, the step's bookkeeping, and either
// row `lim` of the coefficient table (in-cycle step) or the closing coefficients cp
template <bool QUEUED>
__global__ void __launch_bounds__(RED_THREADS) m_coef_kernel(DevState *st, int it, const double *__restrict__ partsB, const double *__restrict__ partsR,
                                                             int nblk, double *__restrict__ hist, int hist_cap, const cplx *__restrict__ den,
                                                             LeanCoef *__restrict__ lcs, MCoef *__restrict__ coef, int lim, int closing, int max_it) {
    __shared__ double lds[2 * 17];
    __shared__ cplx sbeta[LND];
    const int j = blockIdx.x;
    if constexpr (QUEUED) {   // stopped, or at its own last step: m_finish_kernel<true> has done the bookkeeping
        if (!col_active<true>(st, j, (int)gridDim.x, it, max_it)) return;
    } else {   // one workgroup per column, so j < k: col_active<false> would add m_active's column test to this form's instructions
        if (st[j].stop_at < st[j].base + it) return;
    }
    LeanCoef *lc = lcs + j;
    for (int d = 0; d < lim; d++) {
        double s[2];
        fold_partials<2>(partsB + (size_t)((j * LND + d) * 2) * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, s, lds);
        if (threadIdx.x == 0) sbeta[d] = cdiv(make_double2(s[0], s[1]), den[j * LND + d]);
    }
    double rr[1];
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, rr, lds);
    if (threadIdx.x == 0) close_step(st + j, it, rr[0], hist + (size_t)j * hist_cap, hist_cap, closing != 0);
    __syncthreads();
    const int m = threadIdx.x;
    if (m < lim) coef->beta[j][m] = sbeta[m];
    if (!closing) {
        if (lim < LND && m <= lim) {   // table row k = lim (build_lean_kernel)
            const int kk = lim;
            cplx a = make_double2(0., 0.);
            if (m == 0) {
                for (int q = 0; q < kk; q++) a = csub(a, cmul(sbeta[q], q == 0 ? make_double2(1., 0.) : lc->t[q]));
                lc->t[kk] = a;
            } else if (m < kk) {
                for (int q = m; q < kk; q++) a = csub(a, cmul(sbeta[q], q == m ? make_double2(1., 0.) : lc->T[q * LND + m]));
                lc->T[kk * LND + m] = a;
            } else {
                lc->T[kk * LND + kk] = make_double2(1., 0.);
            }
        }
    } else if (m < lim) {              // cp (build_close_kernel / close_x_kernel)
        coef->cp[j][m] = lean_close_coef(lc, sbeta, lim, m);
    }
}
// Ap' = Ar - sum_d beta_d Ap_d (d ascending) with the <r,Ap'>, <Ap',Ap'> partials: the loop of build_lean_kernel.  ap_out may be
// slot 0 itself (closing step): a thread reads its rows of every slot before it writes.
template <int KC, bool QUEUED>
__global__ void __launch_bounds__(RED_THREADS) m_build_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef, MPtrs d, int lim,
                                                              const cplx *r, const cplx *ar, cplx *ap_out, int64_t n, int k,
                                                              double *__restrict__ partsA, int max_it) {
    __shared__ double lds[4 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = col_active<QUEUED>(st, c0 + c, k, it, max_it);
        any = any || act[c];
    }
    if (!any) return;
    double v[4 * KC];
#pragma unroll
    for (int s = 0; s < 4 * KC; s++) v[s] = 0.;
    MV_GRID_STRIDE(i, n) {
        cplx av[KC], rv[KC], ac[KC];
        mv_load<KC>(ar, i, k, c0, av);
        mv_load<KC>(r, i, k, c0, rv);
#pragma unroll
        for (int c = 0; c < KC; c++) ac[c] = make_double2(0., 0.);
        for (int q = 0; q < lim; q++) {
            cplx aj[KC];
            mv_load<KC>(d.aps[q], i, k, c0, aj);
#pragma unroll
            for (int c = 0; c < KC; c++)
                if (c0 + c < k) ac[c] = csub(ac[c], cmul(coef->beta[c0 + c][q], aj[c]));
        }
#pragma unroll
        for (int c = 0; c < KC; c++) {
            const cplx an = cadd(av[c], ac[c]);
            if (act[c]) ap_out[i * k + c0 + c] = an;
            const cplx t = cconj_mul(rv[c], an);
            v[4 * c] += t.x; v[4 * c + 1] += t.y;
            const cplx u = cconj_mul(an, an);
            v[4 * c + 2] += u.x; v[4 * c + 3] += u.y;
        }
    }
    const double tot = block_sum_owner<4 * KC>(v, lds);
    const int t = (int)threadIdx.x;
    if (t < 4 * KC && col_active<QUEUED>(st, c0 + t / 4, k, it, max_it)) partsA[(size_t)((c0 + t / 4) * 4 + (t & 3)) * RED_MAX_BLOCKS + blockIdx.x] = tot;
}
// the x / P0 half of the step that closes a cycle (close_x_kernel): x += sum_m cx_m (P0, D_1 ..), P0' = dir - sum_m cp_m (P0, D_1 ..),
// written over slot 0.  No sums: 256-thread workgroups.
template <int KC, bool QUEUED>
__global__ void __launch_bounds__(256) m_close_x_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef,
                                                        const LeanCoef *__restrict__ lc, MPtrs d, int lim, const cplx *dir, cplx *p_out, cplx *x,
                                                        int64_t n, int k, int max_it) {
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = col_active<QUEUED>(st, c0 + c, k, it, max_it);
        any = any || act[c];
    }
    if (!any) return;
    MV_GRID_STRIDE(i, n) {
        cplx xv[KC], dv[KC], pc[KC];
        mv_load<KC>(x, i, k, c0, xv);
        mv_load<KC>(dir, i, k, c0, dv);
#pragma unroll
        for (int c = 0; c < KC; c++) pc[c] = make_double2(0., 0.);
        for (int q = 0; q < lim; q++) {
            cplx pj[KC];
            mv_load<KC>(d.ps[q], i, k, c0, pj);
#pragma unroll
            for (int c = 0; c < KC; c++)
                if (c0 + c < k) {
                    xv[c] = cadd(xv[c], cmul(lc[c0 + c].cx[q], pj[c]));
                    pc[c] = csub(pc[c], cmul(coef->cp[c0 + c][q], pj[c]));
                }
        }
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (act[c]) {
                x[i * k + c0 + c] = xv[c];
                p_out[i * k + c0 + c] = cadd(dv[c], pc[c]);
            }
    }
}
// Where m_pending_x_kernel puts a column's x.  XFlush: back into the x block, at the end of the batched solve — every column takes
// part, and one without pending updates is not written.  The queued solve's retirement (`mask`: bit j = column j retires) writes
// every retiring column, pending updates or not: XFields into the system's Field, XBlock into column j of a work block, for a
// queue whose systems are not whole Fields (QueueHooks: the even-odd queue), from where the hooks take it.  The x block's column
// is then left as it is: nothing reads it again, so the pending updates cannot be applied twice.
struct XFlush {
    static constexpr bool MASKED = false;
    cplx *x;
    __device__ void put(int64_t i, int k, int col, cplx v) const { x[i * k + col] = v; }
};
struct XFields {
    static constexpr bool MASKED = true;
    QFields f;
    __device__ void put(int64_t i, int, int col, cplx v) const { f.x[col][i] = v; }
};
struct XBlock {
    static constexpr bool MASKED = true;
    cplx *__restrict__ out;
    __device__ void put(int64_t i, int k, int col, cplx v) const { out[i * k + col] = v; }
};

// x_j + the x updates still pending for column j (flush_x_kernel): per column its own count; never skipped
template <int KC, typename SINK>
__global__ void __launch_bounds__(256) m_pending_x_kernel(unsigned mask, const DevState *__restrict__ st, const LeanCoef *__restrict__ lc, MPtrs d,
                                                          const cplx *x, SINK to, int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    if constexpr (SINK::MASKED)
        if (((mask >> c0) & ((1u << KC) - 1u)) == 0) return;
    bool sel[KC];
    int np[KC];
    int npmax = 0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        sel[c] = c0 + c < k && (!SINK::MASKED || ((mask >> (c0 + c)) & 1u));
        np[c] = sel[c] ? st[c0 + c].npend : 0;
        if (np[c] > LND) np[c] = LND;
        npmax = np[c] > npmax ? np[c] : npmax;
    }
    if constexpr (!SINK::MASKED)
        if (npmax <= 0) return;
    MV_GRID_STRIDE(i, n) {
        cplx xv[KC];
        mv_load<KC>(x, i, k, c0, xv);
        for (int q = 0; q < npmax; q++) {
            cplx pj[KC];
            mv_load<KC>(d.ps[q], i, k, c0, pj);
#pragma unroll
            for (int c = 0; c < KC; c++)
                if (q < np[c]) xv[c] = cadd(xv[c], cmul(lc[c0 + c].cx[q], pj[c]));
        }
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (SINK::MASKED ? sel[c] : np[c] > 0) to.put(i, k, c0 + c, xv[c]);
    }
}

// r = b - r (resid_sub_kernel), all columns
__global__ void __launch_bounds__(RED_THREADS) m_resid_sub_kernel(cplx *r, const cplx *__restrict__ b, int64_t ne) {
    MV_GRID_STRIDE(e, ne) r[e] = csub(b[e], r[e]);
}

// ------------------------------------------------------------------------------------------------
// queued solve: admit single columns of the block (gcr_queue_run; pass 2 is m_init_partials_kernel<KC, true>).  `mask`: bit j =
// column j takes part
// ------------------------------------------------------------------------------------------------
// admit, pass 1: the system's x and b into column blockIdx.y of the x and b blocks; without x0 also r0 = P0 = b
__global__ void __launch_bounds__(RED_THREADS) q_scatter_kernel(unsigned mask, QFields f, cplx *__restrict__ xb, cplx *__restrict__ bb, cplx *__restrict__ r,
                                                                cplx *__restrict__ p0, int64_t n, int k, int use_x0) {
    const int j = (int)blockIdx.y;
    if (!((mask >> j) & 1u)) return;
    const cplx *bs = f.b[j];
    const cplx *xs = f.x[j];
    MV_GRID_STRIDE(i, n) {
        const cplx bv = bs[i];
        xb[i * k + j] = xs[i];
        bb[i * k + j] = bv;
        if (!use_x0) {
            r[i * k + j] = bv;
            p0[i * k + j] = bv;
        }
    }
}

// admit with x0: r0 = P0 = b - A x0 of the admitted columns; t holds A x0 (sub: resid_sub_kernel's expression) or, for a plain
// Sparse, b - A x0 formed by the apply itself
__global__ void __launch_bounds__(RED_THREADS) q_r0_kernel(unsigned mask, const cplx *__restrict__ t, const cplx *__restrict__ bb, cplx *__restrict__ r,
                                                           cplx *__restrict__ p0, int64_t n, int k, int sub) {
    const int j = (int)blockIdx.y;
    if (!((mask >> j) & 1u)) return;
    MV_GRID_STRIDE(i, n) {
        const cplx v = sub ? csub(bb[i * k + j], t[i * k + j]) : t[i * k + j];
        r[i * k + j] = v;
        p0[i * k + j] = v;
    }
}

// admit, scalar stage (m_reset_kernel + m_init_kernel for one column, one workgroup per column): the column starts at its own step 0
// when the launches count `global` steps
__global__ void __launch_bounds__(RED_THREADS) q_admit_state_kernel(unsigned mask, DevState *st, int global, double tol2, const double *__restrict__ partsN,
                                                                    const double *__restrict__ partsR, int nblk, double *__restrict__ hist, int hist_cap,
                                                                    LeanCoef *__restrict__ lcs, MCoef *__restrict__ coef) {
    __shared__ double lds[17];
    const int j = blockIdx.x;
    if (!((mask >> j) & 1u)) return;
    double b[1], r[1];
    fold_partials<1>(partsN + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, b, lds);
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, r, lds);
    const int t = (int)threadIdx.x;
    const cplx zero = make_double2(0., 0.);
    for (int e = t; e < LND * LND; e += RED_THREADS) lcs[j].T[e] = zero;
    if (t < LND) {
        lcs[j].t[t] = zero;
        lcs[j].cx[t] = zero;
        coef->beta[j][t] = zero;
        coef->cp[j][t] = zero;
    }
    for (int e = 1 + t; e < hist_cap; e += RED_THREADS) hist[(size_t)j * hist_cap + e] = 0.;
    if (t == 0) {
        coef->alpha[j] = zero;
        st[j].stop_at = INT_MAX;
        st[j].base = -global;
        st[j].iter = 0;
        st[j].npend = 0;
        st[j].bnorm2 = b[0];
        st[j].rr = r[0];
        st[j].tol2 = tol2;
        st[j].closed = 0;
        hist[(size_t)j * hist_cap] = sqrt(r[0]) / sqrt(b[0]);
    }
}

// ------------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------------
#define MK(kernel, blocks, block, ...)                                                        \
    do {                                                                                     \
        hipLaunchKernelGGL(kernel, blocks, dim3(block), 0, ctx().stream, __VA_ARGS__);       \
        MGCR_HIP(hipGetLastError());                                                         \
    } while (0)
// ... of a kernel template over the columns per thread: pick(KC) names the instantiation for KC, a std::integral_constant of kc's
// value (1, 2, or 4 for every other kc)
template <typename PICK, typename... AA>
static int launch_kc(int kc, PICK pick, dim3 blocks, int block, AA... args) {
    return dispatch_value<1, 2, 4>(kc, [&](auto KC) -> int {
        MK(pick(KC), blocks, block, args...);
        return MGCR_OK;
    });
}

namespace {
// Device storage of the batched solve.  Kept from solve to solve (as a GcrState keeps its slots) and re-made when n, k, the number of
// slots or the history length change; released by multi_release() (mgcr_finalize).
struct MWork {
    std::vector<void *> ptrs;
    int64_t n = -1;
    int k = 0, storage = 0, cap = 0;
    bool flex = false;
    cplx *r = nullptr, *ar = nullptr, *den = nullptr;
    cplx *z = nullptr;   // a flexible solve's M r on the step that closes a cycle (and the block another operator than a low-precision GCR writes)
    cplx *xq = nullptr, *bq = nullptr;   // the queued solve's x and b blocks (made by its first call at this n and k)
    std::vector<cplx *> ps, aps;
    DevState *st = nullptr;
    LeanCoef *lc = nullptr;
    MCoef *coef = nullptr;
    double *partsA = nullptr, *partsR = nullptr, *partsN = nullptr, *partsB = nullptr, *dhist = nullptr;
    void release() {
        if (ptrs.empty()) return;
        if (ctx().ready) hipStreamSynchronize(ctx().stream);
        for (void *p : ptrs) hipFree(p);
        ptrs.clear();
        ps.clear(); aps.clear();
        xq = bq = z = nullptr;
        n = -1;
    }
    template <typename T>
    int alloc(T **p, size_t count) {
        hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
        if (e != hipSuccess) {
            set_error("batched GCR: hipMalloc of %zu bytes failed: %s", sizeof(T) * count, hipGetErrorString(e));
            return MGCR_ERR_ALLOC;
        }
        ptrs.push_back((void *)*p);
        return MGCR_OK;
    }
    // flex_: the solve is flexible and wants the block z as well (storage made by a flexible solve serves a plain one, not the reverse)
    int prepare(int64_t n_, int k_, int storage_, int cap_, bool flex_ = false) {
        if (n == n_ && k == k_ && storage == storage_ && cap >= cap_ && (flex || !flex_)) return MGCR_OK;
        release();
        const size_t ne = (size_t)n_ * (size_t)k_;
        ps.assign((size_t)storage_, nullptr);
        aps.assign((size_t)storage_, nullptr);
        int rc = alloc(&r, ne);
        if (rc == MGCR_OK) rc = alloc(&ar, ne);
        if (rc == MGCR_OK && flex_) rc = alloc(&z, ne);
        for (int s = 0; s < storage_ && rc == MGCR_OK; s++) {
            rc = alloc(&ps[(size_t)s], ne);
            if (rc == MGCR_OK) rc = alloc(&aps[(size_t)s], ne);
        }
        if (rc == MGCR_OK) rc = alloc(&den, (size_t)MV_MAX_K * LND);
        if (rc == MGCR_OK) rc = alloc(&st, (size_t)MV_MAX_K);
        if (rc == MGCR_OK) rc = alloc(&lc, (size_t)MV_MAX_K);
        if (rc == MGCR_OK) rc = alloc(&coef, (size_t)1);
        if (rc == MGCR_OK) rc = alloc(&partsA, (size_t)MV_MAX_K * 4 * RED_MAX_BLOCKS);
        if (rc == MGCR_OK) rc = alloc(&partsR, (size_t)MV_MAX_K * RED_MAX_BLOCKS);
        if (rc == MGCR_OK) rc = alloc(&partsN, (size_t)MV_MAX_K * RED_MAX_BLOCKS);
        if (rc == MGCR_OK) rc = alloc(&partsB, (size_t)MV_MAX_K * LND * 2 * RED_MAX_BLOCKS);
        if (rc == MGCR_OK) rc = alloc(&dhist, (size_t)k_ * cap_);
        if (rc != MGCR_OK) { release(); return rc; }
        n = n_; k = k_; storage = storage_; cap = cap_; flex = flex_;
        return MGCR_OK;
    }
    int prepare_queue() {
        if (xq && bq) return MGCR_OK;
        const size_t ne = (size_t)n * (size_t)k;
        int rc = alloc(&xq, ne);
        if (rc == MGCR_OK) rc = alloc(&bq, ne);
        if (rc != MGCR_OK) release();
        return rc;
    }
};
MWork g_work;

// One lockstep solve in flight, what gcr_multi_run and gcr_queue_run share: the work storage as a solve finds it, the launch geometry,
// and the step.
struct MRun {
    MWork &wk = g_work;
    Op *A = nullptr;
    Op *M = nullptr;          // the flexible right preconditioner (gcr_multi_run only), or nullptr
    int64_t n = 0;
    int k = 0, max_it = 0, cap = 0;
    int g = 0, gx = 0;        // blocks of the RED_THREADS kernels / of the 256-thread ones (m_close_x_kernel, m_pending_x_kernel)
    int kc = 0, groups = 0;   // columns per thread, groups of kc columns (blockIdx.y)
    MPtrs d;
    RowMap rmap;

    dim3 grid_of(int blocks, int z = 1) const { return dim3((unsigned)blocks, (unsigned)groups, (unsigned)z); }

    int setup(Op *A_, int64_t n_, int k_, int storage, int max_it_, Op *M_ = nullptr) {
        A = A_; M = M_; n = n_; k = k_; max_it = max_it_; cap = max_it + 1;
        g = red_grid(n);
        gx = g * 4 > 2048 ? 2048 : g * 4;
        kc = mv_group(k);
        groups = (k + kc - 1) / kc;
        MGCR_TRY(wk.prepare(n, k, storage, cap, M != nullptr));
        hipStream_t stream = ctx().stream;
        MGCR_HIP(hipMemsetAsync(wk.dhist, 0, sizeof(double) * (size_t)k * cap, stream));
        MGCR_HIP(hipMemsetAsync(wk.lc, 0, sizeof(LeanCoef) * MV_MAX_K, stream));
        MGCR_HIP(hipMemsetAsync(wk.coef, 0, sizeof(MCoef), stream));
        for (int j = 0; j < LND; j++) { d.ps[j] = wk.ps[(size_t)(j < storage ? j : 0)]; d.aps[j] = wk.aps[(size_t)(j < storage ? j : 0)]; }
        int64_t reach = 0;
        const Op *b0 = op_matrix(A);   // (a MultiDiracOp deals its rows as the DiracOps of its columns do)
        if (b0 && b0->kind == OP_CSR) reach = b0->csr.reach;
        rmap = make_row_map(n, g, reach);
        return MGCR_OK;
    }

    // Enqueues one step (slot bookkeeping: QueueStep): alpha, the residual update, the bookkeeping of the columns at their last step
    // — after which a step that is the last for all of them ends — the k-wide apply, the beta dots, the coefficients, on a closing
    // step the x / P0 update of the block x, and the build.
    // With a flexible right preconditioner M (step_residual_lean's flexible form, per column): r stays in wk.r — the residual ring is
    // not written —, the direction start D = M r goes where the plain step leaves r', into the slot of the next direction, or into
    // wk.z on the step that closes a cycle; there is no preconditioner behind the last update.
    template <bool QUEUED>
    int step(const QueueStep &s, cplx *x) {
        const int it = s.it, lim = s.lim;
        const DevState *st = wk.st;
        const MCoef *coef = wk.coef;
        const cplx *rin = M || s.cur < 1 ? wk.r : wk.ps[(size_t)s.cur];
        cplx *dslot = s.nxt >= 1 ? wk.ps[(size_t)s.nxt] : (M ? wk.z : wk.r);   // what the new direction is started from
        cplx *rnew = M ? wk.r : dslot;
        MK(m_alpha_kernel, dim3((unsigned)k), RED_THREADS, wk.st, it, (const double *)wk.partsA, g, wk.den, s.cur, wk.lc, wk.coef);
        MGCR_TRY(launch_kc(kc, [](auto KC) { return m_xr_kernel<KC>; }, grid_of(g), RED_THREADS, st, it, coef, (const cplx *)wk.aps[(size_t)s.cur],
                           rin, rnew, n, k, wk.partsR));
        if (s.any_last) MK((m_finish_kernel<QUEUED>), dim3((unsigned)k), RED_THREADS, wk.st, it, (const double *)wk.partsR, g, wk.dhist, cap, max_it);
        if (s.all_last) return MGCR_OK;
        if (M) MGCR_TRY(precondition(it, dslot));
        MGCR_TRY(op_apply_multi_raw(A, dslot, wk.ar, n, k));
        constexpr int NDT = 2;
        MGCR_TRY(launch_kc(kc, [](auto KC) { return m_dot_kernel<KC, NDT>; }, grid_of(g, (lim + NDT - 1) / NDT), RED_THREADS, (const cplx *)wk.ar, d,
                           lim, n, k, rmap, wk.partsB));
        MK((m_coef_kernel<QUEUED>), dim3((unsigned)k), RED_THREADS, wk.st, it, (const double *)wk.partsB, (const double *)wk.partsR, g, wk.dhist, cap,
           (const cplx *)wk.den, wk.lc, wk.coef, lim, s.closing ? 1 : 0, max_it);
        if (s.closing)
            MGCR_TRY(launch_kc(kc, [](auto KC) { return m_close_x_kernel<KC, QUEUED>; }, grid_of(gx), 256, st, it, coef, (const LeanCoef *)wk.lc, d,
                               lim, (const cplx *)dslot, wk.ps[0], x, n, k, max_it));
        MGCR_TRY(launch_kc(kc, [](auto KC) { return m_build_kernel<KC, QUEUED>; }, grid_of(g), RED_THREADS, st, it, coef, d, lim, (const cplx *)rnew,
                           (const cplx *)wk.ar, wk.aps[(size_t)s.nxt], n, k, wk.partsA, max_it));
        return MGCR_OK;
    }

    // D = M r behind outer step `it`'s residual update (flex_precond_apply of gcr.hip, per column), into the columns of `out` that are
    // active at that step: a frozen column's slot holds x updates that are still pending.  A low-precision GCR runs as the k-wide
    // lockstep inner solve, handed the columns' states (MFlexGate: the inner solves of frozen columns, and of columns about to end on
    // this residual, are cut to 0 steps); every other operator is applied k-wide into wk.z, whose active columns are then copied.
    // it == 0: the start, out == wk.z — every column takes part, nothing is gated (gcr_start applies M the same way).
    int precondition(int it, cplx *out) {
        if (M->kind == OP_GCR32) {
            const MFlexGate gate{wk.st, it, wk.partsR, g};
            return gcr32_apply_multi_raw(M, wk.r, out, n, k, it > 0 ? &gate : nullptr);
        }
        MGCR_TRY(op_apply_multi_raw(M, wk.r, wk.z, n, k));
        if (out != wk.z) MGCR_TRY(mflex_take(wk.st, it, wk.z, out, n, k, gx));
        return MGCR_OK;
    }
};

// A finished column's iteration count, flag and history row `row` (nullptr: not fetched, the caller wants neither history nor lines)
// as system s of the caller's arrays, and its verbose lines
void report_column(const mgcr_gcr_param &p, int s, int it, const double *row, double *hist, int hist_cap, int *n_iter, int *converged) {
    if (n_iter) n_iter[s] = it;
    if (converged) converged[s] = it == p.max_iter ? 0 : 1;
    if (hist && row)
        for (int i = 0; i <= it && i < hist_cap; i++) hist[(size_t)s * hist_cap + i] = row[i];
    if (p.verbose && row)
        for (int i = 0; i <= it; i++) printf("[%d] Step %d residual norm = %.10e\n", s, i, row[i]);
}
}  // namespace

void mvec_release();   // mvec.hip
void multi_release() {
    g_work.release();
    eo_queue_release();
    mvec_release();
}

static int64_t g_multi_solves = 0, g_multi_flex_solves = 0;
int64_t gcr_multi_solve_count() { return g_multi_solves; }
int64_t gcr_multi_flex_solve_count() { return g_multi_flex_solves; }

int gcr_multi_run(Op *A, const mgcr_gcr_param &p, const cplx *rhs, cplx *x, int64_t n, int k, double *hist, int hist_cap, int *n_iter,
                  int *converged) {
    Context &c = ctx();
    // mode selection of gcr_prepare (gcr.hip)
    const int restart = p.restart;
    int storage = restart;
    if (p.max_iter >= 1 && p.max_iter + 1 < storage) storage = p.max_iter + 1;
    MGCR_CHECK(storage <= LND, MGCR_ERR_UNSUPPORTED, "batched GCR: restart cycles of at most %d steps (the lean cycle) are supported", LND);
    const int max_it = p.max_iter > 0 ? p.max_iter : 1;
    Op *M = p.flexible ? (Op *)p.right_precond : nullptr;   // (the entry point lets no other preconditioner through)
    MRun run;
    MGCR_TRY(run.setup(A, n, k, storage, max_it, M));
    MWork &wk = run.wk;
    const int g = run.g, kc = run.kc, cap = run.cap;
    const size_t ne = (size_t)n * (size_t)k;
    cplx *r = wk.r;

    MK(m_reset_kernel, dim3(1), MV_MAX_K, wk.st, p.tol * p.tol, k);
    // r0 = b, or b - A x0 formed as the single solve forms it (op_residual_raw: one pass for a plain Sparse, apply then b - r for
    // a DiracOp and for a MultiDiracOp)
    if (p.use_x0) {
        if (A->kind == OP_CSR && A->csr.nrow == n && A->csr.ncol == n) {
            MGCR_TRY(op_apply_multi_raw(A, x, r, n, k, rhs));
        } else {
            MGCR_TRY(op_apply_multi_raw(A, x, r, n, k));
            MK(m_resid_sub_kernel, dim3((unsigned)red_grid((int64_t)ne)), RED_THREADS, r, rhs, (int64_t)ne);
        }
    } else {
        MGCR_TRY(mv_copy(r, rhs, n, k));
    }
    if (M) {                                                    // flexible: Z = M r0, P0 = Z, Ap0 = A P0 (gcr.hip start_vectors)
        MGCR_TRY(run.precondition(0, wk.z));
        MGCR_TRY(mv_copy(wk.ps[0], wk.z, n, k));
        MGCR_TRY(op_apply_multi_raw(A, wk.ps[0], wk.aps[0], n, k));
    } else {
        MGCR_TRY(mv_copy(wk.ps[0], r, n, k));                   // P0 = r0
        MGCR_TRY(op_apply_multi_raw(A, r, wk.aps[0], n, k));    // Ap0
    }
    MGCR_TRY(launch_kc(kc, [](auto KC) { return m_init_partials_kernel<KC, false>; }, run.grid_of(g), RED_THREADS, rhs, (const cplx *)r,
                       (const cplx *)wk.aps[0], n, k, wk.partsN, wk.partsR, wk.partsA, 0u, (cplx *)nullptr));
    MK(m_init_kernel, dim3((unsigned)k), RED_THREADS, wk.st, (const double *)wk.partsN, (const double *)wk.partsR, g, wk.dhist, cap);

    const int check_every = p.check_every > 0 ? p.check_every : 10;
    std::vector<DevState> hs((size_t)MV_MAX_K);
    auto poll = [&]() -> int {
        MGCR_HIP(hipMemcpyAsync(hs.data(), wk.st, sizeof(DevState) * MV_MAX_K, hipMemcpyDeviceToHost, c.stream));
        MGCR_HIP(hipStreamSynchronize(c.stream));
        return MGCR_OK;
    };
    int iter_count = 0, cur = 0, global = 0, last_check = 0;
    bool done = false;
    while (global < max_it && !done) {
        global++;
        const bool last = global == max_it;   // every column's last step: the step ends with the bookkeeping
        // slot bookkeeping of gcr.hip's gcr_step
        iter_count++;
        const int lim = storage < iter_count ? storage : iter_count;
        int ic_next = iter_count;
        if (iter_count % restart == 0) ic_next = 0;
        const int nxt = ic_next % storage;
        MGCR_TRY(run.step<false>(QueueStep{global, lim, cur, nxt, ic_next == 0, last, last}, x));
        iter_count = ic_next;
        cur = nxt;
        if (global / check_every != last_check || global == max_it) {
            last_check = global / check_every;
            MGCR_TRY(poll());
            done = true;
            for (int j = 0; j < k; j++) done = done && hs[(size_t)j].stop_at != INT_MAX;
        }
    }
    MGCR_TRY(launch_kc(kc, [](auto KC) { return m_pending_x_kernel<KC, XFlush>; }, run.grid_of(run.gx), 256, 0u, (const DevState *)wk.st,
                       (const LeanCoef *)wk.lc, run.d, (const cplx *)x, XFlush{x}, n, k));
    MGCR_TRY(poll());
    std::vector<double> hh((size_t)k * cap);
    MGCR_HIP(hipMemcpy(hh.data(), wk.dhist, sizeof(double) * hh.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < k; j++) report_column(p, j, hs[(size_t)j].iter, hh.data() + (size_t)j * cap, hist, hist_cap, n_iter, converged);
    g_multi_solves++;
    if (M) g_multi_flex_solves++;
    return resident_check();
}

// ------------------------------------------------------------------------------------------------
// Queued batched solve: nsys systems stream through k = min(width, nsys) columns of ONE batched solve.  The schedule — when the
// host polls, which slots it retires and refills — is queue_plan.h's; this driver carries it out.  Every launch is enqueued by
// the host in stream order: no kernel waits on another workgroup, on a flag or on the host.
//   retire (slots found stopped by a poll): m_pending_x_kernel<KC, XFields> (pending x updates + unpack into the system's Field),
//     the history row and the iteration count go to the system's entries;
//   admit (phase 0 of the cycle, `global` steps launched): q_scatter_kernel; with x0 the k-wide apply into the free `ar` block and
//     q_r0_kernel; the k-wide apply of r into `ar` (column j has the bits of the single apply: Rule 1) and
//     m_init_partials_kernel<KC, true>, which copies the admitted columns into slot 0 while it takes their four start sums;
//     q_admit_state_kernel (base = -global).
//     Per admission point: 2 (3 with x0) passes over the block + 1 (2) k-wide applies, whatever the number of columns admitted.
//   step: gcr_multi_run's (MRun::step), in its QUEUED form: a column at its OWN last step takes the finishing bookkeeping and is
//     left out of what follows.
// ks != nullptr: system s is (1 - ks[s] D) x = b, D = A a plain Sparse; the slots' shifts live in a MultiDiracOp made here, whose
// values travel in the kernel arguments of every apply (KCols): admitting system s into slot j sets entry j.
// hk != nullptr (the even-odd queue, evenodd_queue.hip): the systems are not Fields of n entries.  The hooks fill the admitted
// columns in place of q_scatter_kernel and take the retiring columns from a work block that the XBlock form of m_pending_x_kernel writes in place of
// the XFields one; rhs, x and ks are not read, and the counters that move are the hooks' own.  Without hooks every launch is what it was.
// ------------------------------------------------------------------------------------------------
static int64_t g_queue_solves = 0, g_queue_admissions = 0, g_queue_steps = 0;
static int64_t g_hooked_solves = 0, g_hooked_admissions = 0, g_hooked_steps = 0;
int64_t gcr_queue_stat(int which) {
    return which == 0 ? g_queue_solves : which == 1 ? g_queue_admissions : which == 2 ? g_queue_steps
         : which == 3 ? g_hooked_solves : which == 4 ? g_hooked_admissions : g_hooked_steps;
}

int gcr_queue_run(Op *A0, const mgcr_gcr_param &p, int width, int nsys, const cplx *const *rhs, cplx *const *x, const cplx *ks, int64_t n,
                  double *hist, int hist_cap, int *n_iter, int *converged, QueueHooks *hk) {
    Context &c = ctx();
    const int restart = p.restart;
    QueuePlan qp(width < nsys ? width : nsys, nsys, restart, p.max_iter, p.check_every);
    const int storage = qp.storage, max_it = qp.max_it, k = qp.width;
    MGCR_CHECK(storage <= LND, MGCR_ERR_UNSUPPORTED, "batched GCR: restart cycles of at most %d steps (the lean cycle) are supported", LND);
    Op shifted;   // ks: the slots' MultiDiracOp (borrows A0; lives for this call)
    Op *A = A0;
    if (ks) {
        shifted.kind = OP_DIRAC_MULTI;
        shifted.dim = A0->dim;
        shifted.nrow = A0->nrow;
        shifted.base = A0;
        shifted.nk = k;
        for (int j = 0; j < MV_MAX_K; j++) shifted.ks[j] = make_double2(j < k ? 1. : 0., 0.);
        A = &shifted;
    }
    MRun run;
    MGCR_TRY(run.setup(A, n, k, storage, max_it));
    MWork &wk = run.wk;
    MGCR_TRY(wk.prepare_queue());
    const int g = run.g, kc = run.kc, cap = run.cap;
    cplx *r = wk.r, *ar = wk.ar, *xb = wk.xq, *bb = wk.bq;
    DevState *st = wk.st;
    const bool residual_form = A->kind == OP_CSR && A->csr.nrow == n && A->csr.ncol == n;   // b - A x0 in one pass (op_residual_raw)

    MK(m_reset_kernel, dim3(1), MV_MAX_K, st, p.tol * p.tol, 0);   // every slot empty
    std::vector<DevState> hs((size_t)MV_MAX_K);
    std::vector<double> row;
    QFields f{};
    int64_t admissions0 = qp.admissions;
    int64_t &steps = hk ? g_hooked_steps : g_queue_steps;
    for (;;) {
        if (qp.poll_due()) {
            MGCR_HIP(hipMemcpyAsync(hs.data(), st, sizeof(DevState) * MV_MAX_K, hipMemcpyDeviceToHost, c.stream));
            MGCR_HIP(hipStreamSynchronize(c.stream));
            qp.polled();
            unsigned mask = 0;
            for (int j = 0; j < k; j++)
                if (qp.occupied(j) && hs[(size_t)j].stop_at != INT_MAX) mask |= 1u << j;
            if (mask) {
                if (hk)
                    MGCR_TRY(launch_kc(kc, [](auto KC) { return m_pending_x_kernel<KC, XBlock>; }, run.grid_of(run.gx), 256, mask,
                                       (const DevState *)st, (const LeanCoef *)wk.lc, run.d, (const cplx *)xb, XBlock{hk->retire_block()}, n, k));
                else
                    MGCR_TRY(launch_kc(kc, [](auto KC) { return m_pending_x_kernel<KC, XFields>; }, run.grid_of(run.gx), 256, mask,
                                       (const DevState *)st, (const LeanCoef *)wk.lc, run.d, (const cplx *)xb, XFields{f}, n, k));
                for (int j = 0; j < k; j++) {
                    if (!((mask >> j) & 1u)) continue;
                    const int it = hs[(size_t)j].iter;
                    const bool fetch = (hist && hist_cap > 0) || p.verbose;   // (the row is final: the column stopped before the poll's synchronise)
                    if (fetch) {
                        row.resize((size_t)cap);
                        MGCR_HIP(hipMemcpy(row.data(), wk.dhist + (size_t)j * cap, sizeof(double) * (size_t)(it + 1), hipMemcpyDeviceToHost));
                    }
                    report_column(p, qp.sys[j], it, fetch ? row.data() : nullptr, hist, hist_cap, n_iter, converged);
                    qp.retire(j);
                }
                if (hk) MGCR_TRY(hk->retire(mask));
            }
        }
        int slots[QP_MAX_WIDTH], systems[QP_MAX_WIDTH];
        const int m = qp.admit(slots, systems);
        if (m > 0) {
            unsigned mask = 0;
            for (int i = 0; i < m; i++) {
                const int j = slots[i], s = systems[i];
                mask |= 1u << j;
                if (hk) continue;
                f.b[j] = rhs[s];
                f.x[j] = x[s];
                if (ks) shifted.ks[j] = ks[s];
            }
            const dim3 cols((unsigned)g, (unsigned)k);
            if (hk) MGCR_TRY(hk->admit(mask, m, slots, systems, xb, bb, r, wk.ps[0], p.use_x0 != 0));
            else MK(q_scatter_kernel, cols, RED_THREADS, mask, f, xb, bb, r, wk.ps[0], n, k, p.use_x0 ? 1 : 0);
            if (p.use_x0) {
                if (residual_form) MGCR_TRY(op_apply_multi_raw(A, xb, ar, n, k, bb));
                else MGCR_TRY(op_apply_multi_raw(A, xb, ar, n, k));
                MK(q_r0_kernel, cols, RED_THREADS, mask, (const cplx *)ar, (const cplx *)bb, r, wk.ps[0], n, k, residual_form ? 0 : 1);
            }
            MGCR_TRY(op_apply_multi_raw(A, r, ar, n, k));
            MGCR_TRY(launch_kc(kc, [](auto KC) { return m_init_partials_kernel<KC, true>; }, run.grid_of(g), RED_THREADS, (const cplx *)bb,
                               (const cplx *)r, (const cplx *)ar, n, k, wk.partsN, wk.partsR, wk.partsA, mask, wk.aps[0]));
            MK(q_admit_state_kernel, dim3((unsigned)k), RED_THREADS, mask, st, qp.global, p.tol * p.tol, (const double *)wk.partsN,
               (const double *)wk.partsR, g, wk.dhist, cap, wk.lc, wk.coef);
        }
        if (qp.finished()) break;
        MGCR_CHECK(qp.any_running(), MGCR_ERR_HIP, "queued GCR: a column is still marked as running after its last step");
        steps++;
        MGCR_TRY(run.step<true>(qp.step(), xb));
    }
    MGCR_HIP(hipStreamSynchronize(c.stream));   // the last retirement's writes to the systems' Fields
    (hk ? g_hooked_admissions : g_queue_admissions) += qp.admissions - admissions0;
    (hk ? g_hooked_solves : g_queue_solves)++;
    return resident_check();
}

}  // namespace mgcr
