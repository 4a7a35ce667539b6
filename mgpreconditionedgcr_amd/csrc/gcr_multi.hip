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
};
MWork g_work;
}  // namespace

void mvec_release();   // mvec.hip
void multi_release() {
    g_work.release();
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

}  // namespace mgcr
