// The even-odd preconditioned operator with a dense BLOCK PER SITE on its diagonal (mgcr_eo_create_block; clover-type operators, a
// mass matrix, a local potential, block Poisson): sites are runs of bs consecutive rows, A = B - c H with B block diagonal — one
// bs x bs complex block per site, built from the stored entries inside a site — and H the stored entries between different sites,
// two-colourable on the SITE graph (evenodd_plan.h, evenodd_plan_build_block).  Dirac form: A = 1 - k D, B_s = I - k D_ss, c = k;
// matrix form: A = M itself, B_s = D_ss, c = -1.  The Schur system on the even half is
//     S x_e = bhat_e,   S = B_e - c^2 H_eo B_o^-1 H_oe,   bhat_e = b_e + c H_eo (B_o^-1 b_o),   x_o = B_o^-1 (b_o + c H_oe x_e).
// The operator is an OP_DIRAC_EO whose EoState has has_block set (has_diag stays false): evenodd.hip's eo_apply, eo_schur_step,
// eo_prepare, eo_reconstruct and mgcr_eo_set_k hand over to the functions of this file.
//
// The apply is four launches, whatever the storage of the halves:
//     t = H_oe x (csr_apply);   u = invB_o (.) t (blk_mul_kernel);   v = H_eo u (csr_apply, into the work Field W_UE);
//     y = B_e (.) x - c2 v (blk_combine_kernel<0>)
// and inside a GCR step the last one also takes the step's beta dot products (blk_combine_kernel<1 .. FND>): row map, per-thread
// accumulation order, block sum and partial layout of diag_stage2_kernel, so the folds that follow consume the partials unchanged.
// The inverses of the odd blocks are formed on the device (blk_invert_kernel: Gauss-Jordan with partial pivoting on [B | I] in LDS)
// and the host reads ONE status word per mgcr_eo_set_k — the only synchronisation here.
//
// The bit rules (Rules 1b - 4b of include/mgcr.h): every complex product is (ar br - ai bi, ar bi + ai br), nothing is fused,
// 1 / a = (ar / den, -ai / den) with den = ar ar + ai ai, and a block-vector product (B (.) x)_i is B_i0 x_0, then + B_ij x_j for
// j = 1 .. bs - 1 ascending, real and imaginary parts accumulated separately.
#include <algorithm>
#include <cmath>
#include <string>

#include "internal.h"
#include "reduce.h"
#include "spmv_dev.h"
#include "gcr_dev.h"
#include "evenodd_plan.h"
#include "evenodd_state.h"

namespace mgcr {

static int64_t g_block_applies = 0, g_block_fused_steps = 0;
int64_t eo_block_apply_count() { return g_block_applies; }
int64_t eo_block_fused_step_count() { return g_block_fused_steps; }

void eo_block_destroy(EoState *e) {
    if (!e) return;
    hipFree(e->dblk_even); hipFree(e->dblk_odd); hipFree(e->B_even); hipFree(e->invB_odd); hipFree(e->invB_spare); hipFree(e->blk_status);
    e->dblk_even = e->dblk_odd = e->B_even = e->invB_odd = e->invB_spare = nullptr;
    e->blk_status = nullptr;
}

// ---- the blocks --------------------------------------------------------------------------------------------------------------------
// Layout.  The stored blocks D_ss come from the plan row-major, [sites][bs][bs].  The blocks the applies read (B_e, invB_o) are kept
// with the block COLUMN outermost: entry (r, c) of half-site s at [c * nrows + s * bs + r], nrows = sites * bs the half's rows — the
// thread of half row i then reads M[j * nrows + i], j = 0 .. bs - 1, and the lanes of a wave read consecutive 16-byte entries.
// mgcr_eo_block_diag turns them back into [sites][bs][bs] on the host.
//
// dst = I - k src entry by entry ((1, 0) - k d on the diagonal, (0, 0) - k d off it), or a copy (matrix form); `count` entries of
// blocks of bs x bs, src row-major, dst in the layout above
__global__ void __launch_bounds__(RED_THREADS) blk_coeff_kernel(const cplx *__restrict__ src, cplx *__restrict__ dst, int64_t count, int bs, cplx k,
                                                                int matrix_form) {
    const int bb = bs * bs;
    const int64_t nrows = count / bs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx d = src[i];
        const int64_t site = i / bb;
        const int at = (int)(i - site * bb), r = at / bs, c = at - r * bs;
        cplx out = d;
        if (!matrix_form) {
            const cplx kd = cmul(k, d);
            out = make_double2((r == c ? 1. : 0.) - kd.x, 0. - kd.y);
        }
        dst[(size_t)c * nrows + site * bs + r] = out;
    }
}

constexpr int BLK_INV_SITES = 4;                        // sites per workgroup of blk_invert_kernel, bs lanes each
constexpr int BLK_INV_STRIDE = 2 * EO_BLOCK_MAX + 1;    // entries per LDS row of [B | I]: 2 bs and one of padding (odd: rows on different banks)
constexpr unsigned long long BLK_STATUS_OK = ~0ull;

// io[s] <- io[s]^-1 for `sites` blocks of bs x bs (the layout above), in place: Gauss-Jordan with partial pivoting on [B | I] in LDS, lane r of a site
// owning row r (and, for the swap and the scaling of the pivot row, columns r and bs + r).  For each pivot column p: the row i >= p
// with the largest re^2 + im^2 in column p (the first maximum wins) is swapped into row p, piv = 1 / a_pp, row p is multiplied by
// piv, and every other row i takes row_i - a_ip (.) row_p entry by entry.  A zero or non-finite den of a pivot ends the site's
// elimination and records (site, p) in *status, the smallest (site << 8 | p) of the launch; such a site's block is left as it was.
__global__ void __launch_bounds__(BLK_INV_SITES * EO_BLOCK_MAX) blk_invert_kernel(cplx *__restrict__ io, int64_t sites, int bs,
                                                                                  unsigned long long *__restrict__ status) {
    __shared__ cplx a[BLK_INV_SITES][EO_BLOCK_MAX][BLK_INV_STRIDE];
    __shared__ int failed[BLK_INV_SITES];
    const int ls = (int)threadIdx.x / bs, r = (int)threadIdx.x % bs;   // blockDim.x == BLK_INV_SITES * bs
    const int64_t s = (int64_t)blockIdx.x * BLK_INV_SITES + ls;
    const bool live = ls < BLK_INV_SITES && s < sites;
    cplx(*m)[BLK_INV_STRIDE] = a[live ? ls : 0];
    const size_t nrows = (size_t)sites * bs;
    cplx *blk = io + (size_t)(live ? s : 0) * bs + r;   // entry (r, c) at blk[c * nrows]
    if (live) {
        for (int c = 0; c < bs; c++) {
            m[r][c] = blk[(size_t)c * nrows];
            m[r][bs + c] = make_double2(r == c ? 1. : 0., 0.);
        }
        if (r == 0) failed[ls] = 0;
    }
    __syncthreads();
    for (int p = 0; p < bs; p++) {
        int q = p;
        const bool work = live && !failed[ls];
        if (work) {
            double best = m[p][p].x * m[p][p].x + m[p][p].y * m[p][p].y;
            for (int i = p + 1; i < bs; i++) {
                const double mag = m[i][p].x * m[i][p].x + m[i][p].y * m[i][p].y;
                if (mag > best) { best = mag; q = i; }
            }
        }
        __syncthreads();
        if (work && q != p) {
            const cplx u0 = m[p][r], u1 = m[p][bs + r];
            m[p][r] = m[q][r]; m[p][bs + r] = m[q][bs + r];
            m[q][r] = u0; m[q][bs + r] = u1;
        }
        __syncthreads();
        bool go = work;
        cplx piv = make_double2(0., 0.);
        if (work) {
            const cplx app = m[p][p];
            const double den = app.x * app.x + app.y * app.y;
            if (!(den > 0.) || !isfinite(den)) go = false;
            else piv = make_double2(app.x / den, -app.y / den);
        }
        __syncthreads();   // every lane has read a_pp
        if (work && !go && r == 0) {
            failed[ls] = 1;
            atomicMin(status, ((unsigned long long)s << 8) | (unsigned long long)p);
        }
        if (go) {
            m[p][r] = cmul(m[p][r], piv);
            m[p][bs + r] = cmul(m[p][bs + r], piv);
        }
        __syncthreads();
        if (go && r != p) {
            const cplx f = m[r][p];
            for (int c = 0; c < 2 * bs; c++) m[r][c] = csub(m[r][c], cmul(f, m[p][c]));
        }
        __syncthreads();
    }
    if (live && !failed[ls])
        for (int c = 0; c < bs; c++) blk[(size_t)c * nrows] = m[r][bs + c];
}

// (M (.) x)_i of half row i: row = M + i, its bs block entries nrows apart (half-site i / bs, block row i % bs), x(j) the site's j-th entry
template <typename F>
__device__ __forceinline__ cplx blk_row_product(const cplx *__restrict__ row, size_t nrows, int bs, F &&x) {
    cplx b = row[0], xv = x(0);
    double re = b.x * xv.x - b.y * xv.y, im = b.x * xv.y + b.y * xv.x;
    for (int j = 1; j < bs; j++) {
        b = row[(size_t)j * nrows];
        xv = x(j);
        re = re + (b.x * xv.x - b.y * xv.y);
        im = im + (b.x * xv.y + b.y * xv.x);
    }
    return make_double2(re, im);
}

// t = M (.) u, out of place, one thread per row; skip-aware like the operator applies
__global__ void __launch_bounds__(RED_THREADS) blk_mul_kernel(cplx *__restrict__ t, const cplx *__restrict__ M, const cplx *__restrict__ u, int64_t n,
                                                              int bs, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx *us = u + i / bs * bs;
        t[i] = blk_row_product(M + i, (size_t)n, bs, [&](int j) -> cplx { return us[j]; });
    }
}

// the split of prepare: even[i] = full[ev[i]] and odd = invB_o (.) b_o, the operand gathered through the odd list
__global__ void __launch_bounds__(RED_THREADS) blk_split_scaled_kernel(const cplx *__restrict__ full, cplx *__restrict__ even, cplx *__restrict__ odd,
                                                                       const int32_t *__restrict__ ev, const int32_t *__restrict__ od,
                                                                       const cplx *__restrict__ M, int bs, int64_t ne, int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) {
            even[i] = full[ev[i]];
        } else {
            const int64_t o = i - ne;
            const int32_t *os = od + o / bs * bs;
            odd[o] = blk_row_product(M + o, (size_t)no, bs, [&](int j) -> cplx { return full[os[j]]; });
        }
    }
}
// the merge of reconstruct: full[ev[i]] = even[i], full[od[i]] = (invB_o (.) odd)_i
__global__ void __launch_bounds__(RED_THREADS) blk_merge_scaled_kernel(cplx *__restrict__ full, const cplx *__restrict__ even, const cplx *__restrict__ odd,
                                                                       const int32_t *__restrict__ ev, const int32_t *__restrict__ od,
                                                                       const cplx *__restrict__ M, int bs, int64_t ne, int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) {
            full[ev[i]] = even[i];
        } else {
            const int64_t o = i - ne;
            const cplx *us = odd + o / bs * bs;
            full[od[o]] = blk_row_product(M + o, (size_t)no, bs, [&](int j) -> cplx { return us[j]; });
        }
    }
}

struct BlkDots {
    const cplx *v[FND];
};

// y_i = (B (.) x)_i - c2 v_i and, NDT > 0, the partial sums of <y, Ap_j>, j < NDT: diag_stage2_kernel (evenodd_diag.hip) with the
// row's own term a block-row product and the SpMV's result read from v
template <int NDT>
__global__ void __launch_bounds__(RED_THREADS, (NDT <= 5 ? 8 : 4))
    blk_combine_kernel(const cplx *__restrict__ B, const cplx *__restrict__ x, const cplx *__restrict__ v, cplx c2, cplx *__restrict__ y, BlkDots d,
                       int64_t n, int bs, int nlogical, RowMap rm, double *__restrict__ parts, const int *__restrict__ skip, int skip_it) {
    __shared__ double lds[NDT ? 2 * NDT * 17 : 1];
    if (skip && skip[0] < skip[1] + skip_it) return;
    const int lb = logical_workgroup(rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= nlogical) return;
    int64_t first, last, step;
    row_range(rm, lb, nlogical, n, &first, &last, &step);
    uint32_t i = (uint32_t)first;
    const uint32_t end = (uint32_t)last, stride = (uint32_t)step;
    double acc[NDT ? 2 * NDT : 1];
#pragma unroll
    for (int j = 0; j < 2 * NDT; j++) acc[j] = 0.;
    for (; i < end; i += stride) {
        const cplx *xs = x + i / (uint32_t)bs * (uint32_t)bs;
        const cplx bx = blk_row_product(B + i, (size_t)n, bs, [&](int j) -> cplx { return xs[j]; });
        const cplx yi = csub(bx, cmul(c2, v[i]));
        y[i] = yi;
        if constexpr (NDT > 0) {
            __builtin_amdgcn_sched_barrier(0);
            cplx b[NDT ? NDT : 1];
#pragma unroll
            for (int j = 0; j < NDT; j++) b[j] = ld_stream<true>(d.v[j] + i);
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx u = cconj_mul(yi, b[j]);
                acc[2 * j] += u.x;
                acc[2 * j + 1] += u.y;
            }
        }
    }
    if constexpr (NDT > 0) {
        const double mine = block_sum_owner<2 * NDT>(acc, lds);
        if (threadIdx.x < 2 * NDT) parts[(size_t)threadIdx.x * RED_MAX_BLOCKS + lb] = mine;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int blk_coeff(const EoState *e, const cplx *src, cplx *dst, int64_t sites, cplx k) {
    const int64_t count = sites * e->bs * e->bs;
    if (count == 0) return MGCR_OK;
    return launch(blk_coeff_kernel, (unsigned)red_grid(count), RED_THREADS, 0, src, dst, count, (int)e->bs, k, e->matrix_form ? 1 : 0);
}

// B_o at k into the spare buffer, inverted there; the host then reads the status word (ONE synchronisation).  Success: the spare
// buffer becomes invB_odd — launches already enqueued keep reading the old one, which nothing overwrites before the next call.
// Failure: nothing the operator uses has changed, and *bad_site (a half-site) / *bad_p name the pivot.
static int blk_new_inverse(EoState *e, cplx k, int64_t *bad_site, int *bad_p) {
    *bad_site = -1;
    *bad_p = 0;
    if (e->sites_o == 0) return MGCR_OK;
    unsigned long long st = BLK_STATUS_OK;
    MGCR_HIP(hipMemsetAsync(e->blk_status, 0xff, sizeof st, ctx().stream));   // BLK_STATUS_OK
    MGCR_TRY(blk_coeff(e, e->dblk_odd, e->invB_spare, e->sites_o, k));
    const unsigned grid = (unsigned)((e->sites_o + BLK_INV_SITES - 1) / BLK_INV_SITES);
    MGCR_TRY(launch(blk_invert_kernel, grid, BLK_INV_SITES * (int)e->bs, 0, e->invB_spare, e->sites_o, (int)e->bs, e->blk_status));
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    MGCR_HIP(hipMemcpy(&st, e->blk_status, sizeof st, hipMemcpyDeviceToHost));
    if (st != BLK_STATUS_OK) {
        *bad_site = (int64_t)(st >> 8);
        *bad_p = (int)(st & 0xff);
        return MGCR_OK;
    }
    std::swap(e->invB_odd, e->invB_spare);
    return MGCR_OK;
}
// the full-system row of pivot column p of odd half-site s
static int64_t blk_full_row(const EoState *e, int64_t s, int p) {
    int64_t seen = 0;
    for (int64_t r = 0; r < e->n; r += e->bs)
        if (e->parity[(size_t)r] && seen++ == s) return r + p;
    return -1;
}
static void blk_set_scalars(EoState *e, cplx k) {
    e->k = k;
    e->k2 = host_cmul(k, k);
    e->c = e->matrix_form ? make_double2(-1., 0.) : k;
    e->c2 = host_cmul(e->c, e->c);
    e->cn = make_double2(-e->c.x, -e->c.y);
}

int eo_block_set_k(Op *op, cplx k) {
    EoState *e = op->eo;
    MGCR_CHECK(!e->matrix_form, MGCR_ERR_INVALID,
               "mgcr_eo_set_k: the operator was made in matrix form (mgcr_eo_create_block without k): it has no hopping parameter");
    int64_t bad;
    int p;
    MGCR_TRY(blk_new_inverse(e, k, &bad, &p));
    if (bad >= 0) {
        const int64_t row = blk_full_row(e, bad, p);
        set_error("mgcr_eo_set_k: I - k D_ss of odd site %lld has no inverse (a zero or non-finite pivot in column %d, row %lld): the operator keeps its k",
                  (long long)(row / e->bs), p, (long long)row);
        return MGCR_ERR_INVALID;
    }
    MGCR_TRY(blk_coeff(e, e->dblk_even, e->B_even, e->sites_e, k));   // in stream order: what is enqueued keeps the old B_e
    blk_set_scalars(e, k);
    op->k = k;
    return MGCR_OK;
}

static int blk_mul(const EoState *e, cplx *t, const cplx *u) {
    if (e->no == 0) return MGCR_OK;
    const SkipRef sk = get_apply_skip();
    return launch(blk_mul_kernel, (unsigned)red_grid(e->no), RED_THREADS, 0, t, (const cplx *)e->invB_odd, u, e->no, (int)e->bs, sk.p, sk.it);
}

// y = B_e (.) x - c2 H_eo (invB_o (.) H_oe x); nd > 0: with the partials of <y, vecs_j>
static int blk_schur(EoState *e, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm) {
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "SpMV cannot run in place");
    if (e->ne == 0) return MGCR_OK;
    cplx *u, *v;
    MGCR_TRY(eo_work(e, EoState::W_UO, &u));
    MGCR_TRY(eo_work(e, EoState::W_UE, &v));
    MGCR_TRY(csr_apply(e->half[1]->csr, x, e->t, false, make_double2(0., 0.)));
    MGCR_TRY(blk_mul(e, u, e->t));
    MGCR_TRY(csr_apply(e->half[0]->csr, u, v, false, make_double2(0., 0.)));
    BlkDots d;
    for (int j = 0; j < FND; j++) d.v[j] = nd ? vecs[j < nd ? j : 0] : nullptr;
    const int g = red_grid(e->ne);
    const SkipRef sk = get_apply_skip();
    const cplx *B = e->B_even, *vv = v;
    const cplx c2 = e->c2;
    const int bs = (int)e->bs;
    const int64_t ne = e->ne;
    return dispatch_nd<0, FND>(nd, [&](auto NDT) -> int {
        return launch(blk_combine_kernel<decltype(NDT)::value>, fused_grid(g), RED_THREADS, 0, B, x, vv, c2, y, d, ne, bs, g, rm, parts, sk.p, sk.it);
    });
}

int eo_block_apply(EoState *e, const cplx *x, cplx *y) {
    g_block_applies++;
    return blk_schur(e, x, y, nullptr, 0, nullptr, RowMap{0, 0, 0, 0, 0, 0});
}

// the dot products ride on blk_combine_kernel, which reads no matrix: every storage of the halves takes the fused step
bool eo_block_schur_fusable(const EoState *e) { return e->ne >= 1; }

int eo_block_schur_step(EoState *e, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm) {
    MGCR_CHECK(eo_block_schur_fusable(e), MGCR_ERR_INVALID, "eo_schur_step: an empty even half");
    g_block_applies++;
    g_block_fused_steps++;
    return blk_schur(e, x, y, vecs, nd, parts, rm);
}

// bhat = b_e - cn H_eo (invB_o (.) b_o), cn = -c; b_e stays in W_BE, invB_o (.) b_o in W_BO
int eo_block_prepare(EoState *e, const cplx *b_full, cplx *bhat) {
    cplx *be, *bo;
    MGCR_TRY(eo_work(e, EoState::W_BE, &be));
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    if (e->n)
        MGCR_TRY(launch(blk_split_scaled_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, b_full, be, bo, (const int32_t *)e->d_even,
                        (const int32_t *)e->d_odd, (const cplx *)e->invB_odd, (int)e->bs, e->ne, e->no));
    return eo_shift_apply(e, 0, bo, bhat, e->cn, be);
}

// x_o = invB_o (.) (b_o - cn H_oe x_e), multiplied on its way into x_full
int eo_block_reconstruct(EoState *e, const cplx *b_full, const cplx *xe, cplx *x_full) {
    cplx *bo, *xo;
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    MGCR_TRY(eo_work(e, EoState::W_XO, &xo));
    MGCR_TRY(eo_split(e, b_full, nullptr, bo));
    MGCR_TRY(eo_shift_apply(e, 1, xe, xo, e->cn, bo));
    if (e->n == 0) return MGCR_OK;
    return launch(blk_merge_scaled_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, x_full, xe, (const cplx *)xo, (const int32_t *)e->d_even,
                  (const int32_t *)e->d_odd, (const cplx *)e->invB_odd, (int)e->bs, e->ne, e->no);
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_eo_create_block(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, int32_t bs, const int8_t *parity,
                         const double *k_ri, mgcr_op_t *out) {
    const char *who = "mgcr_eo_create_block";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && n >= 0, MGCR_ERR_INVALID, "%s: null argument", who);
    const bool matrix_form = k_ri == nullptr;
    MGCR_CHECK(matrix_form || k_ri[0] != 0. || k_ri[1] != 0., MGCR_ERR_INVALID, "%s: No k value supplied for Dirac Operator!", who);
    MGCR_CHECK(n < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "%s: matrix dimensions must fit int32 per GPU (got %lld)", who, (long long)n);
    MGCR_CHECK(bs >= 1 && bs <= EO_BLOCK_MAX, MGCR_ERR_INVALID, "%s: block size bs = %d, 1 .. %d are supported", who, (int)bs, (int)EO_BLOCK_MAX);
    MGCR_CHECK(n % bs == 0, MGCR_ERR_INVALID, "%s: n = %lld rows are no whole number of sites of bs = %d rows", who, (long long)n, (int)bs);
    // one row per site: the site diagonal, the operator of mgcr_eo_create_diag on its code path (Rule 4b)
    if (bs == 1) return mgcr_eo_create_diag(n, rowptr, col, val_ri, parity, k_ri, out);
    EvenOddPlan plan;
    std::vector<double> be, bo;
    std::string err;
    if (!evenodd_plan_build_block(n, rowptr, col, val_ri, bs, parity, &plan, &be, &bo, nullptr, &err)) {
        set_error("%s: %s", who, err.c_str());
        return MGCR_ERR_INVALID;
    }
    LOCK();
    EoState *e = new EoState();
    auto fail = [&](int rc) { eo_destroy(e); return rc; };
    e->n = n; e->ne = (int64_t)plan.even.size(); e->no = (int64_t)plan.odd.size(); e->nnz = rowptr[n];
    e->parity = plan.parity;
    e->has_block = true;
    e->matrix_form = matrix_form;
    e->bs = bs;
    e->sites_e = e->ne / bs;
    e->sites_o = e->no / bs;
    const cplx k = matrix_form ? make_double2(0., 0.) : make_double2(k_ri[0], k_ri[1]);
    blk_set_scalars(e, k);
    int brc = eo_build_halves(e, plan, who);
    if (brc != MGCR_OK) return fail(brc);
    const size_t se = be.size() / 2, so = bo.size() / 2;
    hipError_t rc = hipMalloc((void **)&e->dblk_even, sizeof(cplx) * (se ? se : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->dblk_odd, sizeof(cplx) * (so ? so : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->B_even, sizeof(cplx) * (se ? se : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->invB_odd, sizeof(cplx) * (so ? so : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->invB_spare, sizeof(cplx) * (so ? so : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->blk_status, sizeof(unsigned long long));
    if (rc == hipSuccess && se) rc = hipMemcpy(e->dblk_even, be.data(), sizeof(cplx) * se, hipMemcpyHostToDevice);
    if (rc == hipSuccess && so) rc = hipMemcpy(e->dblk_odd, bo.data(), sizeof(cplx) * so, hipMemcpyHostToDevice);
    if (rc != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(rc));
        return fail(MGCR_ERR_ALLOC);
    }
    int64_t bad;
    int p;
    brc = blk_new_inverse(e, k, &bad, &p);
    if (brc != MGCR_OK) return fail(brc);
    if (bad >= 0) {
        const int64_t row = blk_full_row(e, bad, p);
        set_error("%s: the block of odd site %lld has no inverse (a zero or non-finite pivot in column %d, row %lld, of %s)", who,
                  (long long)(row / bs), p, (long long)row, matrix_form ? "D_ss" : "I - k D_ss");
        return fail(MGCR_ERR_INVALID);
    }
    brc = blk_coeff(e, e->dblk_even, e->B_even, e->sites_e, k);
    if (brc != MGCR_OK) return fail(brc);
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC_EO;
    op->dim = op->nrow = e->ne;
    op->k = e->k;
    op->eo = e;
    *out = op;
    return MGCR_OK;
}

int mgcr_eo_block_info(mgcr_op_t eo, int32_t *bs, int64_t *sites_even, int64_t *sites_odd) {
    MGCR_CHECK(eo && eo->kind == OP_DIRAC_EO && eo->eo, MGCR_ERR_INVALID, "mgcr_eo_block_info: not an even-odd preconditioned DiracOp");
    const EoState *e = eo->eo;
    if (bs) *bs = e->has_block ? e->bs : 1;
    if (sites_even) *sites_even = e->has_block ? e->sites_e : e->ne;
    if (sites_odd) *sites_odd = e->has_block ? e->sites_o : e->no;
    return MGCR_OK;
}

int mgcr_eo_block_diag(mgcr_op_t eo, double *B_even_ri, double *invB_odd_ri) {
    const char *who = "mgcr_eo_block_diag";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(eo && eo->kind == OP_DIRAC_EO && eo->eo, MGCR_ERR_INVALID, "%s: not an even-odd preconditioned DiracOp", who);
    LOCK();
    const EoState *e = eo->eo;
    if (!e->has_block) return mgcr_eo_diag(eo, B_even_ri, invB_odd_ri);   // blocks of one entry: a_e and 1 / a_o
    const size_t se = (size_t)e->sites_e * e->bs * e->bs, so = (size_t)e->sites_o * e->bs * e->bs;
    MGCR_CHECK((B_even_ri || se == 0) && (invB_odd_ri || so == 0), MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    // device layout (block column outermost) -> [sites][bs][bs] row-major
    const cplx *src[2] = {e->B_even, e->invB_odd};
    double *dst[2] = {B_even_ri, invB_odd_ri};
    const size_t cnt[2] = {se, so};
    std::vector<cplx> tmp;
    for (int h = 0; h < 2; h++) {
        if (!cnt[h]) continue;
        tmp.resize(cnt[h]);
        MGCR_HIP(hipMemcpy(tmp.data(), src[h], sizeof(cplx) * cnt[h], hipMemcpyDeviceToHost));
        const size_t bs = (size_t)e->bs, nrows = cnt[h] / bs;
        for (size_t i = 0; i < nrows; i++)
            for (size_t c = 0; c < bs; c++) {
                dst[h][2 * (i * bs + c)] = tmp[c * nrows + i].x;
                dst[h][2 * (i * bs + c) + 1] = tmp[c * nrows + i].y;
            }
    }
    return MGCR_OK;
}

}  // extern "C"
