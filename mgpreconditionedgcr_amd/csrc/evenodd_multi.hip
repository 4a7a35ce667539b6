// Even-odd hopping-parameter scans, OP_DIRAC_EO_MULTI: the Schur complements S_j = 1 - k_j^2 D_eo D_oe of ONE hopping matrix on
// column j of a block of exactly nk half-length Fields (multi_dev.h has the layout).  The operator borrows the two half matrices
// and the index lists of an even-odd preconditioned DiracOp (evenodd.hip, evenodd_state.h): nothing is copied or planned again.
//
// Every piece is the k-wide form of its counterpart in evenodd.hip, and column j of each has that counterpart's bits on column j
// with EvenOddDiracOp(D, k_j) (Rule 1 of include/mgcr.h):
//     apply        T = D_oe X;  Y_j = X_j - k_j^2 (D_eo T)_j    two csr_apply_multi launches (spmm.hip), the second with the
//                                                               squares as per-column shifts (KCols) and w = X
//     prepare      Bhat_j = B_e,j - (-k_j) (D_eo B_o)_j
//     reconstruct  X_o,j = B_o,j - (-k_j) (D_oe X_e)_j, then the merge
// The squares are formed on the host by host_cmul, as mgcr_eo_set_k forms its one; values and squares travel in the kernel
// arguments of each launch.  A half that keeps long rows in a CSR tail is multiplied unshifted into a work block and subtracted in a
// launch of its own (eom_sub_scaled_kernel), for eo_shift_apply's reason: the tail kernels subtract their part of a row in a second
// step, which rounds differently.
// The batched GCR (gcr_multi.hip) reaches the apply through op_apply_multi_raw and needs nothing else: plain row map, its own
// m_dot_kernel passes for the beta dot products (schur_step_apply_kernel, the single solve's fused stage 2, has no k-wide form;
// it produces the bits of the plain stage 2 followed by the dot products, so Rule 2 holds all the same).
#include <algorithm>

#include "evenodd_multi.h"

namespace mgcr {

void eo_multi_destroy(EoMultiState *m) {
    if (!m) return;
    hipFree(m->t);
    for (cplx *w : m->work) hipFree(w);
    delete m;
}
int64_t eo_multi_nnz(const EoMultiState *m) { return m && m->eo ? eo_nnz(m->eo->eo) : -1; }

static int eom_block(cplx **slot, int64_t rows, int k) {
    if (!*slot) {
        const size_t count = (size_t)(rows ? rows : 1) * (size_t)k;
        hipError_t rc = hipMalloc((void **)slot, sizeof(cplx) * count);
        MGCR_CHECK(rc == hipSuccess, MGCR_ERR_ALLOC, "MultiEvenOddDiracOp: hipMalloc of a work block failed: %s", hipGetErrorString(rc));
    }
    return MGCR_OK;
}
int eom_work(Op *op, EoState::Work which, cplx **out) {
    const EoState *e = op->eom->eo->eo;
    const bool odd = which == EoState::W_BO || which == EoState::W_XO || which == EoState::W_UO;
    MGCR_TRY(eom_block(&op->eom->work[which], odd ? e->no : e->ne, op->nk));
    *out = op->eom->work[which];
    return MGCR_OK;
}

// full[list[i] * k + c] <-> half[i * k + c].  KP = the power of two from k on: KP neighbouring lanes move the 16 k contiguous bytes of
// a row, one 128-bit access each (lanes from k on idle) — an indexed gather on the full side, a stream on the half side; the row's
// list entry is one load that the group shares.  Either half may be absent in the split.
template <int KP>
__global__ void __launch_bounds__(RED_THREADS) eom_split_kernel(const cplx *__restrict__ full, cplx *__restrict__ even, cplx *__restrict__ odd,
                                                                const int32_t *__restrict__ ev, const int32_t *__restrict__ od, int64_t ne,
                                                                int64_t no, int k) {
    constexpr int ROWS = RED_THREADS / KP;   // rows per workgroup and trip
    const int c = (int)threadIdx.x & (KP - 1);
    if (c >= k) return;
    for (int64_t i = (int64_t)blockIdx.x * ROWS + (int)threadIdx.x / KP; i < ne + no; i += (int64_t)gridDim.x * ROWS) {
        if (i < ne) {
            if (even) even[i * k + c] = full[(int64_t)ev[i] * k + c];
        } else if (odd) {
            odd[(i - ne) * k + c] = full[(int64_t)od[i - ne] * k + c];
        }
    }
}
template <int KP>
__global__ void __launch_bounds__(RED_THREADS) eom_merge_kernel(cplx *__restrict__ full, const cplx *__restrict__ even, const cplx *__restrict__ odd,
                                                                const int32_t *__restrict__ ev, const int32_t *__restrict__ od, int64_t ne,
                                                                int64_t no, int k) {
    constexpr int ROWS = RED_THREADS / KP;
    const int c = (int)threadIdx.x & (KP - 1);
    if (c >= k) return;
    for (int64_t i = (int64_t)blockIdx.x * ROWS + (int)threadIdx.x / KP; i < ne + no; i += (int64_t)gridDim.x * ROWS) {
        if (i < ne) full[(int64_t)ev[i] * k + c] = even[i * k + c];
        else full[(int64_t)od[i - ne] * k + c] = odd[(i - ne) * k + c];
    }
}
// launches kernel<KP> over the rows of the full system
#define EOM_LAUNCH_KP(kernel, e, k, ...)                                                                                         \
    do {                                                                                                                         \
        const int kp__ = (k) <= 1 ? 1 : (k) <= 2 ? 2 : (k) <= 4 ? 4 : (k) <= 8 ? 8 : 16;                                         \
        const unsigned grid__ = (unsigned)red_grid((e)->n * kp__);                                                               \
        if (kp__ == 1) return launch(kernel<1>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 2) return launch(kernel<2>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 4) return launch(kernel<4>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 8) return launch(kernel<8>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        return launch(kernel<16>, grid__, RED_THREADS, 0, __VA_ARGS__);                                                          \
    } while (0)
static int eom_split(const EoState *e, const cplx *full, cplx *even, cplx *odd, int k) {
    if (e->n == 0) return MGCR_OK;
    EOM_LAUNCH_KP(eom_split_kernel, e, k, full, even, odd, (const int32_t *)e->d_even, (const int32_t *)e->d_odd, e->ne, e->no, k);
}
static int eom_merge(const EoState *e, cplx *full, const cplx *even, const cplx *odd, int k) {
    if (e->n == 0) return MGCR_OK;
    EOM_LAUNCH_KP(eom_merge_kernel, e, k, full, even, odd, (const int32_t *)e->d_even, (const int32_t *)e->d_odd, e->ne, e->no, k);
}
#undef EOM_LAUNCH_KP

// y_j = w_j - c_j u_j: eo_sub_scaled_kernel per column.  Rows and columns are dealt as mv_axpy_kernel deals them — a thread carries
// KC neighbouring columns of its rows, gridDim.y column groups
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) eom_sub_scaled_kernel(cplx *__restrict__ y, const cplx *__restrict__ w, KCols cs, const cplx *__restrict__ u,
                                                                     int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    MV_GRID_STRIDE(i, n) {
        cplx wv[KC], uv[KC];
        mv_load<KC>(w, i, k, c0, wv);
        mv_load<KC>(u, i, k, c0, uv);
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (c0 + c < k) y[i * k + c0 + c] = csub(wv[c], cmul(cs.at(c0 + c), uv[c]));
    }
}

// Y_j = W_j - c_j (H X)_j for half H (0: D_eo, 1: D_oe): eo_shift_apply on a block
int eom_shift_apply(Op *op, int h, const cplx *x, cplx *y, const KCols &cs, const cplx *w) {
    const int k = op->nk;
    const CsrDev &A = op->eom->eo->eo->half[h]->csr;
    if (A.nrow == 0) return MGCR_OK;
    if (A.n_tail_rows == 0) return csr_apply_multi(A, x, y, k, true, cs.v[0], &cs, w);
    cplx *u;
    MGCR_TRY(eom_work(op, h == 0 ? EoState::W_UE : EoState::W_UO, &u));
    MGCR_TRY(csr_apply_multi(A, x, u, k, false, make_double2(0., 0.), nullptr, nullptr));
    const int kc = mv_group(k);
    const dim3 grid((unsigned)red_grid(A.nrow), (unsigned)((k + kc - 1) / kc));
    if (kc == 1) hipLaunchKernelGGL(eom_sub_scaled_kernel<1>, grid, dim3(RED_THREADS), 0, ctx().stream, y, w, cs, (const cplx *)u, A.nrow, k);
    else if (kc == 2) hipLaunchKernelGGL(eom_sub_scaled_kernel<2>, grid, dim3(RED_THREADS), 0, ctx().stream, y, w, cs, (const cplx *)u, A.nrow, k);
    else hipLaunchKernelGGL(eom_sub_scaled_kernel<4>, grid, dim3(RED_THREADS), 0, ctx().stream, y, w, cs, (const cplx *)u, A.nrow, k);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

int eo_apply_multi(Op *op, const cplx *x, cplx *y, int64_t n, int k) {
    EoMultiState *m = op->eom;
    MGCR_CHECK(m && m->eo && m->eo->eo, MGCR_ERR_INVALID, "MultiEvenOddDiracOp: no even-odd operator behind it");
    const EoState *e = m->eo->eo;
    MGCR_CHECK(n == e->ne, MGCR_ERR_INVALID, "MultiEvenOddDiracOp: the block must have the %lld rows of the even half", (long long)e->ne);
    MGCR_CHECK(k == op->nk, MGCR_ERR_INVALID, "MultiEvenOddDiracOp carries %d hopping parameters, the block has %d columns", op->nk, k);
    MGCR_TRY(eom_block(&m->t, e->no, k));
    MGCR_TRY(csr_apply_multi(e->half[1]->csr, x, m->t, k, false, make_double2(0., 0.), nullptr, nullptr));
    return eom_shift_apply(op, 0, m->t, y, m->ks2, x);
}

// the factors -k_j of prepare and reconstruct
KCols eom_negated(const Op *op) {
    KCols out;
    for (int q = 0; q < MV_MAX_K; q++) out.v[q] = make_double2(-op->ks[q].x, -op->ks[q].y);
    return out;
}
// Bhat = B_e - (-k_j) (D_eo B_o); the halves of B stay in W_BE, W_BO
static int eom_prepare(Op *op, const cplx *b_full, cplx *bhat) {
    const EoState *e = op->eom->eo->eo;
    cplx *be, *bo;
    MGCR_TRY(eom_work(op, EoState::W_BE, &be));
    MGCR_TRY(eom_work(op, EoState::W_BO, &bo));
    MGCR_TRY(eom_split(e, b_full, be, bo, op->nk));
    return eom_shift_apply(op, 0, bo, bhat, eom_negated(op), be);
}
// X_o = B_o - (-k_j) (D_oe X_e), then X_full = merge(X_e, X_o)
static int eom_reconstruct(Op *op, const cplx *b_full, const cplx *xe, cplx *x_full) {
    const EoState *e = op->eom->eo->eo;
    cplx *bo, *xo;
    MGCR_TRY(eom_work(op, EoState::W_BO, &bo));
    MGCR_TRY(eom_work(op, EoState::W_XO, &xo));
    MGCR_TRY(eom_split(e, b_full, nullptr, bo, op->nk));
    MGCR_TRY(eom_shift_apply(op, 1, xe, xo, eom_negated(op), bo));
    return eom_merge(e, x_full, xe, xo, op->nk);
}

// the values and their squares, checked: no k_j may be zero
static int eom_values(const double *k_ri, int32_t nk, KCols *ks, KCols *ks2, const char *who) {
    for (int q = 0; q < MV_MAX_K; q++) ks->v[q] = ks2->v[q] = make_double2(0., 0.);
    for (int32_t j = 0; j < nk; j++) {
        MGCR_CHECK(k_ri[2 * j] != 0. || k_ri[2 * j + 1] != 0., MGCR_ERR_INVALID, "%s: k[%d] is zero (No k value supplied for Dirac Operator!)", who, (int)j);
        ks->v[j] = make_double2(k_ri[2 * j], k_ri[2 * j + 1]);
        ks2->v[j] = host_cmul(ks->v[j], ks->v[j]);
    }
    return MGCR_OK;
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)
#define EOM_CHECK(op, who)                                                                                             \
    MGCR_CHECK((op) && (op)->kind == OP_DIRAC_EO_MULTI && (op)->eom, MGCR_ERR_INVALID, "%s: not a MultiEvenOddDiracOp", who)
#define EOM_BLOCK(v, rows, who, what)                                                                                                     \
    do {                                                                                                                                  \
        MGCR_CHECK((v)->k == op->nk, MGCR_ERR_INVALID, "%s: the operator carries %d hopping parameters, the %s block has %d columns", who, \
                   op->nk, what, (int)(v)->k);                                                                                            \
        MGCR_CHECK((v)->n == (rows), MGCR_ERR_INVALID, "%s: the %s block has %lld rows, %lld are needed", who, what, (long long)(v)->n,  \
                   (long long)(rows));                                                                                                    \
    } while (0)
// three blocks, pairwise different (blocks of no rows share the null pointer)
#define EOM_DISTINCT3(a, b, c, who)                                                                                                \
    MGCR_CHECK((a) != (b) && (a) != (c) && (b) != (c) && (!(a)->d || ((a)->d != (b)->d && (a)->d != (c)->d)) && (!(b)->d || (b)->d != (c)->d), \
               MGCR_ERR_INVALID, "%s: the three blocks must be different", who)

extern "C" {

int mgcr_eo_multi_create(mgcr_op_t eo, int32_t nk, const double *k_ri, mgcr_op_t *out) {
    const char *who = "mgcr_eo_multi_create";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(eo && k_ri && out, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_CHECK(eo->kind == OP_DIRAC_EO && eo->eo, MGCR_ERR_INVALID, "%s: a MultiEvenOddDiracOp wraps an even-odd preconditioned DiracOp", who);
    MGCR_CHECK(!eo->eo->has_diag, MGCR_ERR_UNSUPPORTED,
               "%s: the operator carries a site diagonal (mgcr_eo_create_diag): 1 - k_j d would differ from column to column, which the scans "
               "do not support; solve one k at a time with mgcr_eo_solve", who);
    MGCR_CHECK(!eo->eo->has_block, MGCR_ERR_UNSUPPORTED,
               "%s: the operator carries a dense block per site (mgcr_eo_create_block): dense site blocks would be per column, which the scans "
               "do not support; solve one k at a time with mgcr_eo_solve", who);
    MGCR_CHECK(nk >= 1 && nk <= MV_MAX_K, MGCR_ERR_INVALID, "%s: nk = %d hopping parameters, 1 .. %d are supported", who, (int)nk, MV_MAX_K);
    KCols ks, ks2;
    MGCR_TRY(eom_values(k_ri, nk, &ks, &ks2, who));
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC_EO_MULTI;
    op->dim = op->nrow = eo->eo->ne;
    op->nk = nk;
    std::copy(ks.v, ks.v + MV_MAX_K, op->ks);
    op->eom = new EoMultiState();
    op->eom->eo = eo;
    op->eom->ks2 = ks2;
    *out = op;
    return MGCR_OK;
}

// The values and their squares travel in the kernel arguments of every launch: what is already enqueued keeps the old ones.
int mgcr_eo_multi_set_k(mgcr_op_t op, const double *k_ri) {
    const char *who = "mgcr_eo_multi_set_k";
    EOM_CHECK(op, who);
    MGCR_CHECK(k_ri, MGCR_ERR_INVALID, "%s: null argument", who);
    KCols ks, ks2;
    MGCR_TRY(eom_values(k_ri, op->nk, &ks, &ks2, who));
    LOCK();
    std::copy(ks.v, ks.v + MV_MAX_K, op->ks);
    op->eom->ks2 = ks2;
    return MGCR_OK;
}

int mgcr_eo_multi_split(mgcr_op_t op, mgcr_mvec_t full, mgcr_mvec_t even, mgcr_mvec_t odd) {
    const char *who = "mgcr_eo_multi_split";
    MGCR_TRY(require_ctx());
    EOM_CHECK(op, who);
    MGCR_CHECK(full && even && odd, MGCR_ERR_INVALID, "%s: null argument", who);
    const EoState *e = op->eom->eo->eo;
    EOM_BLOCK(full, e->n, who, "full");
    EOM_BLOCK(even, e->ne, who, "even");
    EOM_BLOCK(odd, e->no, who, "odd");
    EOM_DISTINCT3(full, even, odd, who);
    LOCK();
    return eom_split(e, full->d, even->d, odd->d, op->nk);
}

int mgcr_eo_multi_merge(mgcr_op_t op, mgcr_mvec_t even, mgcr_mvec_t odd, mgcr_mvec_t full) {
    const char *who = "mgcr_eo_multi_merge";
    MGCR_TRY(require_ctx());
    EOM_CHECK(op, who);
    MGCR_CHECK(full && even && odd, MGCR_ERR_INVALID, "%s: null argument", who);
    const EoState *e = op->eom->eo->eo;
    EOM_BLOCK(full, e->n, who, "full");
    EOM_BLOCK(even, e->ne, who, "even");
    EOM_BLOCK(odd, e->no, who, "odd");
    EOM_DISTINCT3(full, even, odd, who);
    LOCK();
    return eom_merge(e, full->d, even->d, odd->d, op->nk);
}

int mgcr_eo_multi_prepare(mgcr_op_t op, mgcr_mvec_t B_full, mgcr_mvec_t Bhat_even) {
    const char *who = "mgcr_eo_multi_prepare";
    MGCR_TRY(require_ctx());
    EOM_CHECK(op, who);
    MGCR_CHECK(B_full && Bhat_even, MGCR_ERR_INVALID, "%s: null argument", who);
    const EoState *e = op->eom->eo->eo;
    EOM_BLOCK(B_full, e->n, who, "full");
    EOM_BLOCK(Bhat_even, e->ne, who, "even");
    MGCR_CHECK(B_full != Bhat_even && (!B_full->d || B_full->d != Bhat_even->d), MGCR_ERR_INVALID, "%s: the two blocks must be different", who);
    LOCK();
    return eom_prepare(op, B_full->d, Bhat_even->d);
}

int mgcr_eo_multi_reconstruct(mgcr_op_t op, mgcr_mvec_t B_full, mgcr_mvec_t X_even, mgcr_mvec_t X_full) {
    const char *who = "mgcr_eo_multi_reconstruct";
    MGCR_TRY(require_ctx());
    EOM_CHECK(op, who);
    MGCR_CHECK(B_full && X_even && X_full, MGCR_ERR_INVALID, "%s: null argument", who);
    const EoState *e = op->eom->eo->eo;
    EOM_BLOCK(B_full, e->n, who, "right-hand side");
    EOM_BLOCK(X_even, e->ne, who, "even");
    EOM_BLOCK(X_full, e->n, who, "full");
    EOM_DISTINCT3(B_full, X_even, X_full, who);
    LOCK();
    return eom_reconstruct(op, B_full->d, X_even->d, X_full->d);
}

int mgcr_eo_multi_solve(mgcr_op_t op, const mgcr_gcr_param *param, mgcr_mvec_t B_full, mgcr_mvec_t X_full, double *hist, int32_t hist_cap,
                        int32_t *n_iter, int32_t *converged) {
    const char *who = "mgcr_eo_multi_solve";
    MGCR_TRY(require_ctx());
    EOM_CHECK(op, who);
    MGCR_CHECK(param && B_full && X_full, MGCR_ERR_INVALID, "%s: null argument", who);
    const EoState *e = op->eom->eo->eo;
    EOM_BLOCK(B_full, e->n, who, "right-hand side");
    EOM_BLOCK(X_full, e->n, who, "solution");
    MGCR_CHECK(B_full != X_full && (!X_full->d || B_full->d != X_full->d), MGCR_ERR_INVALID, "rhs and x must be different blocks");
    // (the restrictions of mgcr_gcr_solve_multi, checked before anything is enqueued)
    MGCR_CHECK(param->truncation >= 0 && param->restart >= 0 && param->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_CHECK(param->truncation == 0, MGCR_ERR_UNSUPPORTED, "%s: truncation mode is not supported (restart mode only)", who);
    MGCR_CHECK(param->restart != 0, MGCR_ERR_UNSUPPORTED, "%s: restart mode only (restart != 0)", who);
    MGCR_CHECK(!param->left_precond && !param->right_precond, MGCR_ERR_UNSUPPORTED, "%s: preconditioners are not supported", who);
    MGCR_CHECK(!param->flexible && !param->profile_spmv, MGCR_ERR_UNSUPPORTED, "%s: flexible / profile_spmv are not supported", who);
    LOCK();
    cplx *bhat, *xe;
    MGCR_TRY(eom_work(op, EoState::W_BHAT, &bhat));
    MGCR_TRY(eom_work(op, EoState::W_XE, &xe));
    MGCR_TRY(eom_prepare(op, B_full->d, bhat));
    MGCR_TRY(eom_split(e, X_full->d, xe, nullptr, op->nk));   // x_e on entry is the even half of X_full, as in mgcr_eo_solve
    MGCR_TRY(gcr_multi_run(op, *param, bhat, xe, e->ne, op->nk, hist, hist_cap, n_iter, converged));
    return eom_reconstruct(op, B_full->d, xe, X_full->d);
}

}  // extern "C"
