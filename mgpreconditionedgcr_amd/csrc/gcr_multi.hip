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

// The queued solve (gcr_queue_run) admits columns at different steps, so a column's LAST step (own step number == max_iter) is not the
// launch's: such a column takes the finishing bookkeeping (q_finish_kernel, which freezes it with stop_at == its step number) while
// its neighbours run a full step, and the kernels behind that bookkeeping — coefficients, closing x update, build — must leave it
// alone although stop_at == base + it reads as active.  Those three have q_ TWINS (q_coef_kernel, q_build_kernel, q_close_x_kernel):
// the m_ kernel with this test in place of m_active.  A change to the arithmetic of either twin belongs in both — the bit-for-bit
// rule ties solve_multi and solve_queue to the same single solve.  They are copies because a body shared through an inlined
// __device__ function compiles to other code for the m_ entries (the work-group size is then looked up, not assumed).
__device__ __forceinline__ bool q_active(const DevState *st, int col, int k, int it, int max_it) {
    return m_active(st, col, k, it) && st[col].base + it < max_it;
}

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

// |b|^2, |r|^2, <r,Ap>, <Ap,Ap> per column in one pass (norm_partials_kernel, norm_partials_kernel, dot2_partials_kernel)
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) m_init_partials_kernel(const cplx *__restrict__ b, const cplx *__restrict__ r,
                                                                      const cplx *__restrict__ ap, int64_t n, int k, double *__restrict__ partsN,
                                                                      double *__restrict__ partsR, double *__restrict__ partsA) {
    __shared__ double lds[6 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
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
        if (col < k) {
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

// the last step a solve can run: bookkeeping only (finish_step_kernel)
__global__ void __launch_bounds__(RED_THREADS) m_finish_kernel(DevState *st, int it, const double *__restrict__ partsR, int nblk,
                                                               double *__restrict__ hist, int hist_cap) {
    __shared__ double lds[17];
    const int j = blockIdx.x;
    if (st[j].stop_at < st[j].base + it) return;
    double rr[1];
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, rr, lds);
    if (threadIdx.x == 0) close_step(st + j, it, rr[0], hist + (size_t)j * hist_cap, hist_cap, false);
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

// (twin: q_coef_kernel below)
// the prologue of build_lean_kernel / build_close_kernel, one workgroup per column: betas, the step's bookkeeping, and either
// row `lim` of the coefficient table (in-cycle step) or the closing coefficients cp
__global__ void __launch_bounds__(RED_THREADS) m_coef_kernel(DevState *st, int it, const double *__restrict__ partsB, const double *__restrict__ partsR,
                                                             int nblk, double *__restrict__ hist, int hist_cap, const cplx *__restrict__ den,
                                                             LeanCoef *__restrict__ lcs, MCoef *__restrict__ coef, int lim, int closing) {
    __shared__ double lds[2 * 17];
    __shared__ cplx sbeta[LND];
    const int j = blockIdx.x;
    if (st[j].stop_at < st[j].base + it) return;
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
// ... in the queued solve (the same kernel but for the test of the column's own last step)
__global__ void __launch_bounds__(RED_THREADS) q_coef_kernel(DevState *st, int it, const double *__restrict__ partsB, const double *__restrict__ partsR,
                                                             int nblk, double *__restrict__ hist, int hist_cap, const cplx *__restrict__ den,
                                                             LeanCoef *__restrict__ lcs, MCoef *__restrict__ coef, int lim, int closing, int max_it) {
    __shared__ double lds[2 * 17];
    __shared__ cplx sbeta[LND];
    const int j = blockIdx.x;
    if (!q_active(st, j, (int)gridDim.x, it, max_it)) return;   // stopped, or at its own last step: q_finish_kernel has done the bookkeeping
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

// (twin: q_build_kernel below)
// Ap' = Ar - sum_d beta_d Ap_d (d ascending) with the <r,Ap'>, <Ap',Ap'> partials: the loop of build_lean_kernel.  ap_out may be
// slot 0 itself (closing step): a thread reads its rows of every slot before it writes.
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) m_build_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef, MPtrs d, int lim,
                                                              const cplx *r, const cplx *ar, cplx *ap_out, int64_t n, int k,
                                                              double *__restrict__ partsA) {
    __shared__ double lds[4 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = m_active(st, c0 + c, k, it);
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
    if (t < 4 * KC && m_active(st, c0 + t / 4, k, it)) partsA[(size_t)((c0 + t / 4) * 4 + (t & 3)) * RED_MAX_BLOCKS + blockIdx.x] = tot;
}
// ... in the queued solve
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) q_build_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef, MPtrs d, int lim,
                                                              const cplx *r, const cplx *ar, cplx *ap_out, int64_t n, int k,
                                                              double *__restrict__ partsA, int max_it) {
    __shared__ double lds[4 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = q_active(st, c0 + c, k, it, max_it);
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
    if (t < 4 * KC && q_active(st, c0 + t / 4, k, it, max_it)) partsA[(size_t)((c0 + t / 4) * 4 + (t & 3)) * RED_MAX_BLOCKS + blockIdx.x] = tot;
}

// (twin: q_close_x_kernel below)
// the x / P0 half of the step that closes a cycle (close_x_kernel): x += sum_m cx_m (P0, D_1 ..), P0' = dir - sum_m cp_m (P0, D_1 ..),
// written over slot 0.  No sums: 256-thread workgroups.
template <int KC>
__global__ void __launch_bounds__(256) m_close_x_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef,
                                                        const LeanCoef *__restrict__ lc, MPtrs d, int lim, const cplx *dir, cplx *p_out, cplx *x,
                                                        int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = m_active(st, c0 + c, k, it);
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
// ... in the queued solve
template <int KC>
__global__ void __launch_bounds__(256) q_close_x_kernel(const DevState *__restrict__ st, int it, const MCoef *__restrict__ coef,
                                                        const LeanCoef *__restrict__ lc, MPtrs d, int lim, const cplx *dir, cplx *p_out, cplx *x,
                                                        int64_t n, int k, int max_it) {
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = q_active(st, c0 + c, k, it, max_it);
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

// the x updates still pending when the solve ends (flush_x_kernel): per column its own count; never skipped
template <int KC>
__global__ void __launch_bounds__(256) m_flush_kernel(const DevState *__restrict__ st, const LeanCoef *__restrict__ lc, MPtrs d, cplx *x, int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    int np[KC];
    int npmax = 0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        np[c] = c0 + c < k ? st[c0 + c].npend : 0;
        if (np[c] > LND) np[c] = LND;
        npmax = np[c] > npmax ? np[c] : npmax;
    }
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
            if (np[c] > 0) x[i * k + c0 + c] = xv[c];
    }
}

// r = b - r (resid_sub_kernel), all columns
__global__ void __launch_bounds__(RED_THREADS) m_resid_sub_kernel(cplx *r, const cplx *__restrict__ b, int64_t ne) {
    MV_GRID_STRIDE(e, ne) r[e] = csub(b[e], r[e]);
}

// ------------------------------------------------------------------------------------------------
// queued solve: retire / admit single columns of the block (gcr_queue_run).  `mask`: bit j = column j takes part
// ------------------------------------------------------------------------------------------------
struct QFields {   // per column: the system's Fields (by value in the kernel arguments)
    const cplx *b[MV_MAX_K];
    cplx *x[MV_MAX_K];
};

// a column's own last step: the bookkeeping of m_finish_kernel, then the column is frozen
__global__ void __launch_bounds__(RED_THREADS) q_finish_kernel(DevState *st, int it, int max_it, const double *__restrict__ partsR, int nblk,
                                                               double *__restrict__ hist, int hist_cap) {
    __shared__ double lds[17];
    const int j = blockIdx.x;
    if (st[j].stop_at < st[j].base + it || st[j].base + it != max_it) return;
    double rr[1];
    fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, rr, lds);
    if (threadIdx.x == 0) {
        close_step(st + j, it, rr[0], hist + (size_t)j * hist_cap, hist_cap, false);
        st[j].stop_at = st[j].base + it;
    }
}

// retire: x_s = column j of the x block + the column's pending updates (the expression of m_flush_kernel), written to the system's
// Field.  The block's column is left as it is: nothing reads it again, so the pending updates cannot be applied twice.
template <int KC>
__global__ void __launch_bounds__(256) q_retire_kernel(unsigned mask, const DevState *__restrict__ st, const LeanCoef *__restrict__ lc, MPtrs d,
                                                       const cplx *__restrict__ x, QFields f, int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    if (((mask >> c0) & ((1u << KC) - 1u)) == 0) return;
    bool ret[KC];
    int np[KC];
    int npmax = 0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        ret[c] = c0 + c < k && ((mask >> (c0 + c)) & 1u);
        np[c] = ret[c] ? st[c0 + c].npend : 0;
        if (np[c] > LND) np[c] = LND;
        npmax = np[c] > npmax ? np[c] : npmax;
    }
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
            if (ret[c]) f.x[c0 + c][i] = xv[c];
    }
}

// ... for a queue whose systems are not whole Fields (QueueHooks: the even-odd queue): the same expression, written to column j of a
// work block, from where the hooks take it
template <int KC>
__global__ void __launch_bounds__(256) hq_retire_kernel(unsigned mask, const DevState *__restrict__ st, const LeanCoef *__restrict__ lc, MPtrs d,
                                                        const cplx *__restrict__ x, cplx *__restrict__ out, int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    if (((mask >> c0) & ((1u << KC) - 1u)) == 0) return;
    bool ret[KC];
    int np[KC];
    int npmax = 0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        ret[c] = c0 + c < k && ((mask >> (c0 + c)) & 1u);
        np[c] = ret[c] ? st[c0 + c].npend : 0;
        if (np[c] > LND) np[c] = LND;
        npmax = np[c] > npmax ? np[c] : npmax;
    }
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
            if (ret[c]) out[i * k + c0 + c] = xv[c];
    }
}

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

// admit, pass 2: A r0 (the k-wide apply left it in ar) into slot 0 of the admitted columns, and their four start sums — rows per
// thread and summation tree of m_init_partials_kernel.  A continuing column's sums (the closing step's build wrote them) stay.
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) q_admit_kernel(unsigned mask, const cplx *__restrict__ b, const cplx *__restrict__ r,
                                                              const cplx *__restrict__ ar, cplx *__restrict__ ap0, int64_t n, int k,
                                                              double *__restrict__ partsN, double *__restrict__ partsR, double *__restrict__ partsA) {
    __shared__ double lds[6 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    if (((mask >> c0) & ((1u << KC) - 1u)) == 0) return;   // (uniform over the workgroup)
    bool adm[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) adm[c] = c0 + c < k && ((mask >> (c0 + c)) & 1u);
    double v[6 * KC];
#pragma unroll
    for (int s = 0; s < 6 * KC; s++) v[s] = 0.;
    MV_GRID_STRIDE(i, n) {
        cplx bv[KC], rv[KC], av[KC];
        mv_load<KC>(b, i, k, c0, bv);
        mv_load<KC>(r, i, k, c0, rv);
        mv_load<KC>(ar, i, k, c0, av);
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (adm[c]) ap0[i * k + c0 + c] = av[c];
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
        if (col < k && ((mask >> col) & 1u)) {
            if (s < 4) partsA[(size_t)(col * 4 + s) * RED_MAX_BLOCKS + blockIdx.x] = tot;
            else if (s == 4) partsN[(size_t)col * RED_MAX_BLOCKS + blockIdx.x] = tot;
            else partsR[(size_t)col * RED_MAX_BLOCKS + blockIdx.x] = tot;
        }
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
#define MK(kernel, grid, block, ...)                                                         \
    do {                                                                                     \
        hipLaunchKernelGGL(kernel, grid, dim3(block), 0, ctx().stream, __VA_ARGS__);         \
        MGCR_HIP(hipGetLastError());                                                         \
    } while (0)
#define MK_KC(kernel, g, block, ...)                                                         \
    do {                                                                                     \
        const dim3 grid__((unsigned)(g), (unsigned)groups);                                  \
        if (kc == 1) MK((kernel<1>), grid__, block, __VA_ARGS__);                            \
        else if (kc == 2) MK((kernel<2>), grid__, block, __VA_ARGS__);                       \
        else MK((kernel<4>), grid__, block, __VA_ARGS__);                                    \
    } while (0)

namespace {
// Device storage of the batched solve.  Kept from solve to solve (as a GcrState keeps its slots) and re-made when n, k, the number of
// slots or the history length change; released by multi_release() (mgcr_finalize).
struct MWork {
    std::vector<void *> ptrs;
    int64_t n = -1;
    int k = 0, storage = 0, cap = 0;
    cplx *r = nullptr, *ar = nullptr, *den = nullptr;
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
        xq = bq = nullptr;
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
    int prepare(int64_t n_, int k_, int storage_, int cap_) {
        if (n == n_ && k == k_ && storage == storage_ && cap >= cap_) return MGCR_OK;
        release();
        const size_t ne = (size_t)n_ * (size_t)k_;
        ps.assign((size_t)storage_, nullptr);
        aps.assign((size_t)storage_, nullptr);
        int rc = alloc(&r, ne);
        if (rc == MGCR_OK) rc = alloc(&ar, ne);
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
        n = n_; k = k_; storage = storage_; cap = cap_;
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
}  // namespace

void mvec_release();   // mvec.hip
void multi_release() {
    g_work.release();
    eo_queue_release();
    mvec_release();
}

static int64_t g_multi_solves = 0;
int64_t gcr_multi_solve_count() { return g_multi_solves; }

int gcr_multi_run(Op *A, const mgcr_gcr_param &p, const cplx *rhs, cplx *x, int64_t n, int k, double *hist, int hist_cap, int *n_iter,
                  int *converged) {
    Context &c = ctx();
    // mode selection of gcr_prepare (gcr.hip)
    const int restart = p.restart;
    int storage = restart;
    if (p.max_iter >= 1 && p.max_iter + 1 < storage) storage = p.max_iter + 1;
    MGCR_CHECK(storage <= LND, MGCR_ERR_UNSUPPORTED, "batched GCR: restart cycles of at most %d steps (the lean cycle) are supported", LND);
    const int max_it = p.max_iter > 0 ? p.max_iter : 1;
    const int cap = max_it + 1;
    const int g = red_grid(n);
    const int kc = mv_group(k), groups = (k + kc - 1) / kc;
    const size_t ne = (size_t)n * (size_t)k;
    MWork &wk = g_work;
    MGCR_TRY(wk.prepare(n, k, storage, cap));
    cplx *r = wk.r, *ar = wk.ar, *den = wk.den;
    std::vector<cplx *> &ps = wk.ps, &aps = wk.aps;
    DevState *st = wk.st;
    LeanCoef *lc = wk.lc;
    MCoef *coef = wk.coef;
    double *partsA = wk.partsA, *partsR = wk.partsR, *partsN = wk.partsN, *partsB = wk.partsB, *dhist = wk.dhist;
    MGCR_HIP(hipMemsetAsync(dhist, 0, sizeof(double) * (size_t)k * cap, c.stream));
    MGCR_HIP(hipMemsetAsync(lc, 0, sizeof(LeanCoef) * MV_MAX_K, c.stream));
    MGCR_HIP(hipMemsetAsync(coef, 0, sizeof(MCoef), c.stream));

    MPtrs d;
    for (int j = 0; j < LND; j++) { d.ps[j] = ps[(size_t)(j < storage ? j : 0)]; d.aps[j] = aps[(size_t)(j < storage ? j : 0)]; }
    int64_t reach = 0;
    {
        const Op *b0 = op_matrix(A);   // (a MultiDiracOp deals its rows as the DiracOps of its columns do)
        if (b0 && b0->kind == OP_CSR) reach = b0->csr.reach;
    }
    const RowMap rmap = make_row_map(n, g, reach);

    MK(m_reset_kernel, dim3(1), MV_MAX_K, st, p.tol * p.tol, k);
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
    MGCR_TRY(mv_copy(ps[0], r, n, k));                       // P0 = r0
    MGCR_TRY(op_apply_multi_raw(A, r, aps[0], n, k));        // Ap0
    MK_KC(m_init_partials_kernel, g, RED_THREADS, rhs, (const cplx *)r, (const cplx *)aps[0], n, k, partsN, partsR, partsA);
    MK(m_init_kernel, dim3((unsigned)k), RED_THREADS, st, (const double *)partsN, (const double *)partsR, g, dhist, cap);

    const int check_every = p.check_every > 0 ? p.check_every : 10;
    std::vector<DevState> hs((size_t)MV_MAX_K);
    auto poll = [&]() -> int {
        MGCR_HIP(hipMemcpyAsync(hs.data(), st, sizeof(DevState) * MV_MAX_K, hipMemcpyDeviceToHost, c.stream));
        MGCR_HIP(hipStreamSynchronize(c.stream));
        return MGCR_OK;
    };
    const cplx *rcur = r;
    int iter_count = 0, cur = 0, global = 0, last_check = 0;
    bool done = false;
    while (global < max_it && !done) {
        global++;
        const int it = global;
        const bool last = global == max_it;
        // slot bookkeeping of gcr.hip's gcr_step
        iter_count++;
        const int lim = storage < iter_count ? storage : iter_count;
        int ic_next = iter_count;
        if (iter_count % restart == 0) ic_next = 0;
        const int nxt = ic_next % storage;
        cplx *dslot = nxt >= 1 ? ps[(size_t)nxt] : r;
        MK(m_alpha_kernel, dim3((unsigned)k), RED_THREADS, st, it, (const double *)partsA, g, den, cur, lc, coef);
        MK_KC(m_xr_kernel, g, RED_THREADS, (const DevState *)st, it, (const MCoef *)coef, (const cplx *)aps[(size_t)cur], rcur, dslot, n, k, partsR);
        rcur = dslot;
        if (last) {
            MK(m_finish_kernel, dim3((unsigned)k), RED_THREADS, st, it, (const double *)partsR, g, dhist, cap);
        } else {
            const int closing = ic_next == 0 ? 1 : 0;
            MGCR_TRY(op_apply_multi_raw(A, dslot, ar, n, k));
            {
                constexpr int NDT = 2;
                const dim3 grid((unsigned)g, (unsigned)groups, (unsigned)((lim + NDT - 1) / NDT));
                if (kc == 1) MK((m_dot_kernel<1, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
                else if (kc == 2) MK((m_dot_kernel<2, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
                else MK((m_dot_kernel<4, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
            }
            MK(m_coef_kernel, dim3((unsigned)k), RED_THREADS, st, it, (const double *)partsB, (const double *)partsR, g, dhist, cap,
               (const cplx *)den, lc, coef, lim, closing);
            if (closing)
                MK_KC(m_close_x_kernel, red_grid(n) * 4 > 2048 ? 2048 : red_grid(n) * 4, 256, (const DevState *)st, it, (const MCoef *)coef,
                      (const LeanCoef *)lc, d, lim, (const cplx *)dslot, ps[0], x, n, k);
            MK_KC(m_build_kernel, g, RED_THREADS, (const DevState *)st, it, (const MCoef *)coef, d, lim, rcur, (const cplx *)ar, aps[(size_t)nxt], n, k,
                  partsA);
        }
        iter_count = ic_next;
        cur = nxt;
        if (global / check_every != last_check || global == max_it) {
            last_check = global / check_every;
            MGCR_TRY(poll());
            done = true;
            for (int j = 0; j < k; j++) done = done && hs[(size_t)j].stop_at != INT_MAX;
        }
    }
    MK_KC(m_flush_kernel, red_grid(n) * 4 > 2048 ? 2048 : red_grid(n) * 4, 256, (const DevState *)st, (const LeanCoef *)lc, d, x, n, k);
    MGCR_TRY(poll());
    std::vector<double> hh((size_t)k * cap);
    MGCR_HIP(hipMemcpy(hh.data(), dhist, sizeof(double) * hh.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < k; j++) {
        const int it = hs[(size_t)j].iter;
        if (n_iter) n_iter[j] = it;
        if (converged) converged[j] = it == p.max_iter ? 0 : 1;
        if (hist)
            for (int i = 0; i <= it && i < hist_cap; i++) hist[(size_t)j * hist_cap + i] = hh[(size_t)j * cap + i];
        if (p.verbose) {
            for (int i = 0; i <= it; i++) printf("[%d] Step %d residual norm = %.10e\n", j, i, hh[(size_t)j * cap + i]);
        }
    }
    g_multi_solves++;
    return resident_check();
}

// ------------------------------------------------------------------------------------------------
// Queued batched solve: nsys systems stream through k = min(width, nsys) columns of ONE batched solve.  The schedule — when the
// host polls, which slots it retires and refills — is queue_plan.h's; this driver carries it out.  Every launch is enqueued by
// the host in stream order: no kernel waits on another workgroup, on a flag or on the host.
//   retire (slots found stopped by a poll): q_retire_kernel (pending x updates + unpack into the system's Field), the history
//     row and the iteration count go to the system's entries;
//   admit (phase 0 of the cycle, `global` steps launched): q_scatter_kernel; with x0 the k-wide apply into the free `ar` block and
//     q_r0_kernel; the k-wide apply of r into `ar` (column j has the bits of the single apply: Rule 1) and q_admit_kernel, which
//     copies the admitted columns into slot 0 while it takes their four start sums; q_admit_state_kernel (base = -global).
//     Per admission point: 2 (3 with x0) passes over the block + 1 (2) k-wide applies, whatever the number of columns admitted.
//   step: gcr_multi_run's, except that a column at its OWN last step takes q_finish_kernel and is left out of what follows.
// ks != nullptr: system s is (1 - ks[s] D) x = b, D = A a plain Sparse; the slots' shifts live in a MultiDiracOp made here, whose
// values travel in the kernel arguments of every apply (KCols): admitting system s into slot j sets entry j.
// hk != nullptr (the even-odd queue, evenodd_queue.hip): the systems are not Fields of n entries.  The hooks fill the admitted
// columns in place of q_scatter_kernel and take the retiring columns from a work block that hq_retire_kernel writes in place of
// q_retire_kernel; rhs, x and ks are not read, and the counters that move are the hooks' own.  Without hooks every launch is what it was.
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
    const int cap = max_it + 1;
    const int g = red_grid(n);
    const int kc = mv_group(k), groups = (k + kc - 1) / kc;
    const int gx = red_grid(n) * 4 > 2048 ? 2048 : red_grid(n) * 4;   // the 256-thread kernels (m_close_x_kernel, m_flush_kernel)
    MWork &wk = g_work;
    MGCR_TRY(wk.prepare(n, k, storage, cap));
    MGCR_TRY(wk.prepare_queue());
    cplx *r = wk.r, *ar = wk.ar, *den = wk.den, *xb = wk.xq, *bb = wk.bq;
    std::vector<cplx *> &ps = wk.ps, &aps = wk.aps;
    DevState *st = wk.st;
    LeanCoef *lc = wk.lc;
    MCoef *coef = wk.coef;
    double *partsA = wk.partsA, *partsR = wk.partsR, *partsN = wk.partsN, *partsB = wk.partsB, *dhist = wk.dhist;
    MGCR_HIP(hipMemsetAsync(dhist, 0, sizeof(double) * (size_t)k * cap, c.stream));
    MGCR_HIP(hipMemsetAsync(lc, 0, sizeof(LeanCoef) * MV_MAX_K, c.stream));
    MGCR_HIP(hipMemsetAsync(coef, 0, sizeof(MCoef), c.stream));

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
    MPtrs d;
    for (int j = 0; j < LND; j++) { d.ps[j] = ps[(size_t)(j < storage ? j : 0)]; d.aps[j] = aps[(size_t)(j < storage ? j : 0)]; }
    int64_t reach = 0;
    {
        const Op *b0 = op_matrix(A);
        if (b0 && b0->kind == OP_CSR) reach = b0->csr.reach;
    }
    const RowMap rmap = make_row_map(n, g, reach);
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
                if (hk) MK_KC(hq_retire_kernel, gx, 256, mask, (const DevState *)st, (const LeanCoef *)lc, d, (const cplx *)xb, hk->retire_block(), n, k);
                else MK_KC(q_retire_kernel, gx, 256, mask, (const DevState *)st, (const LeanCoef *)lc, d, (const cplx *)xb, f, n, k);
                for (int j = 0; j < k; j++) {
                    if (!((mask >> j) & 1u)) continue;
                    const int s = qp.sys[j], it = hs[(size_t)j].iter;
                    if (n_iter) n_iter[s] = it;
                    if (converged) converged[s] = it == p.max_iter ? 0 : 1;
                    if ((hist && hist_cap > 0) || p.verbose) {   // (the row is final: the column stopped before the poll's synchronise)
                        row.resize((size_t)cap);
                        MGCR_HIP(hipMemcpy(row.data(), dhist + (size_t)j * cap, sizeof(double) * (size_t)(it + 1), hipMemcpyDeviceToHost));
                        if (hist)
                            for (int i = 0; i <= it && i < hist_cap; i++) hist[(size_t)s * hist_cap + i] = row[(size_t)i];
                        if (p.verbose)
                            for (int i = 0; i <= it; i++) printf("[%d] Step %d residual norm = %.10e\n", s, i, row[(size_t)i]);
                    }
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
            if (hk) MGCR_TRY(hk->admit(mask, m, slots, systems, xb, bb, r, ps[0], p.use_x0 != 0));
            else MK(q_scatter_kernel, cols, RED_THREADS, mask, f, xb, bb, r, ps[0], n, k, p.use_x0 ? 1 : 0);
            if (p.use_x0) {
                if (residual_form) MGCR_TRY(op_apply_multi_raw(A, xb, ar, n, k, bb));
                else MGCR_TRY(op_apply_multi_raw(A, xb, ar, n, k));
                MK(q_r0_kernel, cols, RED_THREADS, mask, (const cplx *)ar, (const cplx *)bb, r, ps[0], n, k, residual_form ? 0 : 1);
            }
            MGCR_TRY(op_apply_multi_raw(A, r, ar, n, k));
            MK_KC(q_admit_kernel, g, RED_THREADS, mask, (const cplx *)bb, (const cplx *)r, (const cplx *)ar, aps[0], n, k, partsN, partsR, partsA);
            MK(q_admit_state_kernel, dim3((unsigned)k), RED_THREADS, mask, st, qp.global, p.tol * p.tol, (const double *)partsN, (const double *)partsR, g,
               dhist, cap, lc, coef);
        }
        if (qp.finished()) break;
        MGCR_CHECK(qp.any_running(), MGCR_ERR_HIP, "queued GCR: a column is still marked as running after its last step");
        const QueueStep s = qp.step();
        steps++;
        const int it = s.it, lim = s.lim;
        const cplx *rin = s.cur >= 1 ? ps[(size_t)s.cur] : r;
        cplx *dslot = s.nxt >= 1 ? ps[(size_t)s.nxt] : r;
        MK(m_alpha_kernel, dim3((unsigned)k), RED_THREADS, st, it, (const double *)partsA, g, den, s.cur, lc, coef);
        MK_KC(m_xr_kernel, g, RED_THREADS, (const DevState *)st, it, (const MCoef *)coef, (const cplx *)aps[(size_t)s.cur], rin, dslot, n, k, partsR);
        if (s.any_last) MK(q_finish_kernel, dim3((unsigned)k), RED_THREADS, st, it, max_it, (const double *)partsR, g, dhist, cap);
        if (s.all_last) continue;
        MGCR_TRY(op_apply_multi_raw(A, dslot, ar, n, k));
        {
            constexpr int NDT = 2;
            const dim3 grid((unsigned)g, (unsigned)groups, (unsigned)((lim + NDT - 1) / NDT));
            if (kc == 1) MK((m_dot_kernel<1, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
            else if (kc == 2) MK((m_dot_kernel<2, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
            else MK((m_dot_kernel<4, NDT>), grid, RED_THREADS, (const cplx *)ar, d, lim, n, k, rmap, partsB);
        }
        MK(q_coef_kernel, dim3((unsigned)k), RED_THREADS, st, it, (const double *)partsB, (const double *)partsR, g, dhist, cap, (const cplx *)den, lc,
           coef, lim, s.closing ? 1 : 0, max_it);
        if (s.closing)
            MK_KC(q_close_x_kernel, gx, 256, (const DevState *)st, it, (const MCoef *)coef, (const LeanCoef *)lc, d, lim, (const cplx *)dslot, ps[0], xb, n,
                  k, max_it);
        MK_KC(q_build_kernel, g, RED_THREADS, (const DevState *)st, it, (const MCoef *)coef, d, lim, (const cplx *)dslot, (const cplx *)ar,
              aps[(size_t)s.nxt], n, k, partsA, max_it);
    }
    MGCR_HIP(hipStreamSynchronize(c.stream));   // the last retirement's writes to the systems' Fields
    (hk ? g_hooked_admissions : g_queue_admissions) += qp.admissions - admissions0;
    (hk ? g_hooked_solves : g_queue_solves)++;
    return resident_check();
}

}  // namespace mgcr
