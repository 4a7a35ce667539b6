// The even-odd preconditioned operator with a SITE DIAGONAL (mgcr_eo_create_diag): A = diag(a) - c H, H the stored off-diagonal part,
// two-colourable as in evenodd.hip.  Dirac form: A = 1 - k D and D stores a diagonal d, so a = (1, 0) - k d and c = k; matrix form:
// A = M itself (Poisson, a Wilson operator written with its mass), a = d and c = -1.  The diagonal blocks are scalars, their inverse
// is element-wise, and the Schur system on the even half is
//     S x_e = bhat_e,   S = diag(a_e) - c^2 H_eo diag(1 / a_o) H_oe,   bhat_e = b_e + c H_eo (b_o / a_o),   x_o = (b_o + c H_oe x_e) / a_o.
// The operator is an OP_DIRAC_EO whose EoState has has_diag set: evenodd.hip's eo_apply, eo_schur_step, eo_prepare and
// eo_reconstruct hand over to the functions of this file, and an operator without a diagonal never comes here.
//
// The apply is two launches where both halves are stored one thread per row (L == 1, no CSR tail; the MODE / WT forms of
// schur_step_apply_kernel):
//     stage 1   t_i = (1 / a_o)_i (H_oe x)_i                     diag_stage1_kernel
//     stage 2   y_i = a_e,i w_i - c2 (H_eo t)_i                  diag_stage2_kernel<.., NDT = 0>
// and inside a GCR step stage 2 also takes the step's beta dot products (NDT = 1 .. FND), exactly as schur_step_apply_kernel does:
// same row map, same per-thread accumulation order, same block sum and partial layout.  A half stored otherwise takes csr_apply and
// an element-wise launch (diag_scale_kernel / diag_combine_kernel), as eo_shift_apply treats a CSR tail.  Every product is formed
// un-fused, (ar br - ai bi, ar bi + ai br): Rules 1d - 3d of include/mgcr.h.
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

static int64_t g_diag_fused_steps = 0;
int64_t eo_diag_fused_step_count() { return g_diag_fused_steps; }

void eo_diag_destroy(EoState *e) {
    if (!e) return;
    hipFree(e->dd_even); hipFree(e->dd_odd); hipFree(e->a_even); hipFree(e->inv_a_odd);
    e->dd_even = e->dd_odd = e->a_even = e->inv_a_odd = nullptr;
}

// ---- a and 1 / a, on the host (the singular check) and on the device (in stream order: what is enqueued keeps the old values) ----
// a = (1, 0) - k d  (Dirac form)  or  d  (matrix form);  1 / a = (ar / den, -ai / den), den = ar ar + ai ai
__host__ __device__ __forceinline__ cplx diag_a(cplx d, cplx k, int matrix_form) {
    if (matrix_form) return d;
    const cplx kd = make_double2(k.x * d.x - k.y * d.y, k.x * d.y + k.y * d.x);
    return make_double2(1. - kd.x, 0. - kd.y);
}
__host__ __device__ __forceinline__ cplx diag_inv(cplx a) {
    const double den = a.x * a.x + a.y * a.y;
    return make_double2(a.x / den, -a.y / den);
}

__global__ void __launch_bounds__(RED_THREADS) diag_coeff_kernel(const cplx *__restrict__ dd_even, const cplx *__restrict__ dd_odd, cplx k,
                                                                 int matrix_form, cplx *__restrict__ a_even, cplx *__restrict__ inv_a_odd,
                                                                 int64_t ne, int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) a_even[i] = diag_a(dd_even[i], k, matrix_form);
        else inv_a_odd[i - ne] = diag_inv(diag_a(dd_odd[i - ne], k, matrix_form));
    }
}

// the full-system row of the first odd site whose 1 / a is exactly zero or not finite; -1: none
static int64_t diag_first_singular(const EoState *e, cplx k, int matrix_form) {
    int64_t bad = -1;
    for (size_t i = 0; i < e->h_d_odd.size() && bad < 0; i++) {
        const cplx v = diag_inv(diag_a(e->h_d_odd[i], k, matrix_form));
        if (!std::isfinite(v.x) || !std::isfinite(v.y) || (v.x == 0. && v.y == 0.)) bad = (int64_t)i;
    }
    if (bad < 0) return -1;
    int64_t seen = 0;
    for (int64_t r = 0; r < e->n; r++)
        if (e->parity[(size_t)r] && seen++ == bad) return r;
    return -1;
}

static int diag_set_coefficients(EoState *e, cplx k) {
    if (e->n == 0) return MGCR_OK;
    return launch(diag_coeff_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, (const cplx *)e->dd_even, (const cplx *)e->dd_odd, k,
                  e->matrix_form ? 1 : 0, e->a_even, e->inv_a_odd, e->ne, e->no);
}

int eo_diag_set_k(Op *op, cplx k) {
    EoState *e = op->eo;
    MGCR_CHECK(!e->matrix_form, MGCR_ERR_INVALID,
               "mgcr_eo_set_k: the operator was made in matrix form (mgcr_eo_create_diag without k): it has no hopping parameter");
    const int64_t bad = diag_first_singular(e, k, 0);   // on the host, before anything is enqueued: a refused k changes nothing
    MGCR_CHECK(bad < 0, MGCR_ERR_INVALID, "mgcr_eo_set_k: 1 - k d of odd row %lld has no inverse (a singular diagonal block): the operator keeps its k",
               (long long)bad);
    MGCR_TRY(diag_set_coefficients(e, k));
    e->k = op->k = k;
    e->k2 = host_cmul(k, k);
    e->c = k;
    e->c2 = e->k2;
    e->cn = make_double2(-k.x, -k.y);
    return MGCR_OK;
}

// ---- element-wise kernels -----------------------------------------------------------------------------------------------------------
// t = s (.) u; t may be u
__global__ void __launch_bounds__(RED_THREADS) diag_scale_kernel(cplx *t, const cplx *__restrict__ s, const cplx *u, int64_t n,
                                                                 const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) t[i] = cmul(s[i], u[i]);
}
// y = a (.) w - c2 u
__global__ void __launch_bounds__(RED_THREADS) diag_combine_kernel(cplx *__restrict__ y, const cplx *__restrict__ a, const cplx *__restrict__ w, cplx c2,
                                                                   const cplx *__restrict__ u, int64_t n, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = csub(cmul(a[i], w[i]), cmul(c2, u[i]));
}
// the split of prepare: even[i] = full[ev[i]] (even may be absent) and odd[i] = s_i full[od[i]] — the 1 / a_o scaling costs no pass
__global__ void __launch_bounds__(RED_THREADS) diag_split_scaled_kernel(const cplx *__restrict__ full, cplx *__restrict__ even, cplx *__restrict__ odd,
                                                                        const int32_t *__restrict__ ev, const int32_t *__restrict__ od,
                                                                        const cplx *__restrict__ s, int64_t ne, int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) {
            if (even) even[i] = full[ev[i]];
        } else {
            odd[i - ne] = cmul(s[i - ne], full[od[i - ne]]);
        }
    }
}
// the merge of reconstruct: full[ev[i]] = even[i], full[od[i]] = s_i odd[i]
__global__ void __launch_bounds__(RED_THREADS) diag_merge_scaled_kernel(cplx *__restrict__ full, const cplx *__restrict__ even, const cplx *__restrict__ odd,
                                                                        const int32_t *__restrict__ ev, const int32_t *__restrict__ od,
                                                                        const cplx *__restrict__ s, int64_t ne, int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) full[ev[i]] = even[i];
        else full[od[i - ne]] = cmul(s[i - ne], odd[i - ne]);
    }
}

// ---- the two stages on a half stored one thread per row --------------------------------------------------------------------------
struct DiagDots {
    const cplx *v[FND];
};
constexpr bool diag_eight_waves(int MODE, int WT, int NDT) { return (MODE == 1 || (MODE == 3 && WT <= 7)) && NDT <= 5; }

// stage 1: t_i = s_i (H x)_i, s = 1 / a_o — the row product of schur_step_apply_kernel, the scale factor streamed in behind the
// row's gathers.  Plain row map.
template <int MODE, int WT>
__global__ void __launch_bounds__(RED_THREADS, (diag_eight_waves(MODE, WT, 0) ? 8 : 4))
    diag_stage1_kernel(RowMat m, const cplx *__restrict__ x, const cplx *__restrict__ s, cplx *__restrict__ t, int64_t n, int nlogical, RowMap rm,
                       const int *__restrict__ skip, int skip_it) {
    extern __shared__ __attribute__((aligned(16))) unsigned char diag_smem[];
    if (skip && skip[0] < skip[1] + skip_it) return;
    const int lb = logical_workgroup(rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= nlogical) return;
    const int32_t W = WT ? WT : m.W;
    int64_t first, last, step;
    row_range(rm, lb, nlogical, n, &first, &last, &step);
    uint32_t i = (uint32_t)first;
    const uint32_t end = (uint32_t)last, stride = (uint32_t)step;
    int32_t t0 = 0;
    if ((MODE == 1 || MODE == 2) && i < end) t0 = (int32_t)__builtin_nontemporal_load(m.pid + i) * W;
    PatLds pl{nullptr, nullptr, nullptr};
    if (MODE == 1) pl = stage_patterns(m, diag_smem);
    for (; i < end; i += stride) {
        int32_t t0_next = 0;
        if ((MODE == 1 || MODE == 2) && i + stride < end) t0_next = (int32_t)__builtin_nontemporal_load(m.pid + i + stride) * W;
        const cplx sum = fused_row_product<MODE, WT>(m, i, t0, pl, [&](int32_t j) -> cplx { return x[j]; });
        const cplx si = ld_stream<true>(s + i);
        t[i] = cmul(si, sum);
        t0 = t0_next;
    }
}

// stage 2: y_i = a_i w_i - c2 (H t)_i (m.k = c2) and, NDT > 0, the partial sums of <y, Ap_j>, j < NDT: schur_step_apply_kernel with
// the row's own term scaled by a_e, one 16-byte stream and one complex product more per row.
template <int MODE, int WT, int NDT>
__global__ void __launch_bounds__(RED_THREADS, (diag_eight_waves(MODE, WT, NDT) ? 8 : 4))
    diag_stage2_kernel(RowMat m, const cplx *__restrict__ t, const cplx *__restrict__ w, const cplx *__restrict__ a, cplx *__restrict__ y, DiagDots d,
                       int64_t n, int nlogical, RowMap rm, double *__restrict__ parts, const int *__restrict__ skip, int skip_it) {
    __shared__ double lds[NDT ? 2 * NDT * 17 : 1];
    extern __shared__ __attribute__((aligned(16))) unsigned char diag_smem[];
    if (skip && skip[0] < skip[1] + skip_it) return;
    const int lb = logical_workgroup(rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= nlogical) return;
    const int32_t W = WT ? WT : m.W;
    int64_t first, last, step;
    row_range(rm, lb, nlogical, n, &first, &last, &step);
    uint32_t i = (uint32_t)first;
    const uint32_t end = (uint32_t)last, stride = (uint32_t)step;
    int32_t t0 = 0;
    if ((MODE == 1 || MODE == 2) && i < end) t0 = (int32_t)__builtin_nontemporal_load(m.pid + i) * W;
    PatLds pl{nullptr, nullptr, nullptr};
    if (MODE == 1) pl = stage_patterns(m, diag_smem);
    double v[NDT ? 2 * NDT : 1];
#pragma unroll
    for (int j = 0; j < 2 * NDT; j++) v[j] = 0.;
    for (; i < end; i += stride) {
        int32_t t0_next = 0;
        if ((MODE == 1 || MODE == 2) && i + stride < end) t0_next = (int32_t)__builtin_nontemporal_load(m.pid + i + stride) * W;
        const cplx sum = fused_row_product<MODE, WT>(m, i, t0, pl, [&](int32_t j) -> cplx { return t[j]; });
        const cplx ai = ld_stream<true>(a + i);
        const cplx yi = csub(cmul(ai, w[i]), cmul(m.k, sum));
        y[i] = yi;
        if constexpr (NDT > 0) {
            __builtin_amdgcn_sched_barrier(0);
            cplx b[NDT ? NDT : 1];
#pragma unroll
            for (int j = 0; j < NDT; j++) b[j] = ld_stream<true>(d.v[j] + i);
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx u = cconj_mul(yi, b[j]);
                v[2 * j] += u.x;
                v[2 * j + 1] += u.y;
            }
        }
        t0 = t0_next;
    }
    if constexpr (NDT > 0) {
        const double mine = block_sum_owner<2 * NDT>(v, lds);
        if (threadIdx.x < 2 * NDT) parts[(size_t)threadIdx.x * RED_MAX_BLOCKS + lb] = mine;
    }
}

// Is the half stored in a form the two kernels above exist for?  (the conditions of eo_schur_fusable, minus the option)
struct DiagRowForm {
    int mode, wt;
    size_t lds;
};
static bool diag_row_form(const CsrDev &A, DiagRowForm *f) {
    if (A.pat_mode == 1 && (int64_t)A.npat * A.W * 20 > 48 * 1024) return false;   // the pattern table must fit LDS
    const bool sten = csr_stencil_active(A);
    if (sten && A.sten_rare) return false;                                         // (no rare-tail form, as in evenodd.hip)
    if (!(A.L == 1 && A.n_tail_rows == 0 && A.nrow >= 1 && A.W >= 1)) return false;
    f->mode = sten ? 3 : (A.pat_mode == 1 || A.pat_mode == 2 ? A.pat_mode : 0);
    f->wt = sten ? (sten_slots(A) != 7 ? 9 : 7) : (A.W == 7 ? 7 : 0);
    f->lds = sten ? 0 : row_mat_lds_bytes(A);
    return true;
}
// f(MODE, WT) for the eight (MODE, WT) pairs of schur_step_apply_kernel
template <typename F>
static int diag_dispatch_form(const DiagRowForm &rf, F &&f) {
    return dispatch_value<3, 1, 2, 0>(rf.mode, [&](auto MODE) -> int {
        return dispatch_value<9, 7, 0>(rf.wt, [&](auto WTT) -> int {
            constexpr int M = decltype(MODE)::value, WW = decltype(WTT)::value;
            if constexpr (M == 3 ? WW != 0 : WW != 9) {
                return f(MODE, WTT);
            } else {
                set_error("even-odd operator with a diagonal: no kernel of this form");
                return MGCR_ERR_INVALID;
            }
        });
    });
}

// t = (1 / a_o) (.) (H_oe x)
static int diag_stage1(EoState *e, const cplx *x) {
    const CsrDev &A = e->half[1]->csr;
    if (A.nrow == 0) return MGCR_OK;
    const SkipRef sk = get_apply_skip();
    DiagRowForm rf;
    if (!diag_row_form(A, &rf)) {
        MGCR_TRY(csr_apply(A, x, e->t, false, make_double2(0., 0.)));
        return launch(diag_scale_kernel, (unsigned)red_grid(A.nrow), RED_THREADS, 0, e->t, (const cplx *)e->inv_a_odd, (const cplx *)e->t, A.nrow, sk.p,
                      sk.it);
    }
    const RowMat m = row_mat(A, false, make_double2(0., 0.));
    const int g = red_grid(A.nrow);
    const RowMap rm{0, 0, 0, 0, 0, 0};
    const cplx *s = e->inv_a_odd;
    cplx *t = e->t;
    return diag_dispatch_form(rf, [&](auto MODE, auto WTT) -> int {
        return launch(diag_stage1_kernel<decltype(MODE)::value, decltype(WTT)::value>, fused_grid(g), RED_THREADS, rf.lds, m, x, s, t, A.nrow, g, rm, sk.p,
                      sk.it);
    });
}

// y = a_e (.) w - c2 (H_eo t), nd == 0; with the partials of <y, vecs_j>, j < nd, else (the half must have a row form then)
static int diag_stage2(EoState *e, const cplx *w, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm) {
    const CsrDev &A = e->half[0]->csr;
    if (A.nrow == 0) return MGCR_OK;
    const SkipRef sk = get_apply_skip();
    DiagRowForm rf;
    if (!diag_row_form(A, &rf)) {
        MGCR_CHECK(nd == 0, MGCR_ERR_INVALID, "eo_schur_step: H_eo is not stored in a form the fused stage exists for");
        cplx *u;
        MGCR_TRY(eo_work(e, EoState::W_UE, &u));
        MGCR_TRY(csr_apply(A, e->t, u, false, make_double2(0., 0.)));
        return launch(diag_combine_kernel, (unsigned)red_grid(A.nrow), RED_THREADS, 0, y, (const cplx *)e->a_even, w, e->c2, (const cplx *)u, A.nrow, sk.p,
                      sk.it);
    }
    const RowMat m = row_mat(A, true, e->c2);
    DiagDots d;
    for (int j = 0; j < FND; j++) d.v[j] = nd ? vecs[j < nd ? j : 0] : nullptr;
    const int g = red_grid(A.nrow);
    const cplx *t = e->t, *a = e->a_even;
    return diag_dispatch_form(rf, [&](auto MODE, auto WTT) -> int {
        return dispatch_nd<0, FND>(nd, [&](auto NDT) -> int {
            return launch(diag_stage2_kernel<decltype(MODE)::value, decltype(WTT)::value, decltype(NDT)::value>, fused_grid(g), RED_THREADS, rf.lds, m, t,
                          w, a, y, d, A.nrow, g, rm, parts, sk.p, sk.it);
        });
    });
}

int eo_diag_apply(EoState *e, const cplx *x, cplx *y) {
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "SpMV cannot run in place");
    MGCR_TRY(diag_stage1(e, x));
    return diag_stage2(e, x, y, nullptr, 0, nullptr, RowMap{0, 0, 0, 0, 0, 0});
}

bool eo_diag_schur_fusable(const EoState *e) {
    DiagRowForm rf;
    return diag_row_form(e->half[0]->csr, &rf);
}

int eo_diag_schur_step(EoState *e, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm) {
    MGCR_CHECK(eo_diag_schur_fusable(e), MGCR_ERR_INVALID, "eo_schur_step: H_eo is not stored in a form the fused stage exists for");
    MGCR_TRY(diag_stage1(e, x));
    g_diag_fused_steps++;
    return diag_stage2(e, x, y, vecs, nd, parts, rm);
}

// bhat = b_e - cn H_eo ((1 / a_o) (.) b_o), cn = -c; b_e stays in W_BE, the scaled b_o in W_BO
int eo_diag_prepare(EoState *e, const cplx *b_full, cplx *bhat) {
    cplx *be, *bo;
    MGCR_TRY(eo_work(e, EoState::W_BE, &be));
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    if (e->n)
        MGCR_TRY(launch(diag_split_scaled_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, b_full, be, bo, (const int32_t *)e->d_even,
                        (const int32_t *)e->d_odd, (const cplx *)e->inv_a_odd, e->ne, e->no));
    return eo_shift_apply(e, 0, bo, bhat, e->cn, be);
}

// x_o = (1 / a_o) (.) (b_o - cn H_oe x_e), scaled on its way into x_full
int eo_diag_reconstruct(EoState *e, const cplx *b_full, const cplx *xe, cplx *x_full) {
    cplx *bo, *xo;
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    MGCR_TRY(eo_work(e, EoState::W_XO, &xo));
    MGCR_TRY(eo_split(e, b_full, nullptr, bo));
    MGCR_TRY(eo_shift_apply(e, 1, xe, xo, e->cn, bo));
    if (e->n == 0) return MGCR_OK;
    return launch(diag_merge_scaled_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, x_full, xe, (const cplx *)xo, (const int32_t *)e->d_even,
                  (const int32_t *)e->d_odd, (const cplx *)e->inv_a_odd, e->ne, e->no);
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_eo_create_diag(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity, const double *k_ri,
                        mgcr_op_t *out) {
    const char *who = "mgcr_eo_create_diag";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && n >= 0, MGCR_ERR_INVALID, "%s: null argument", who);
    const bool matrix_form = k_ri == nullptr;
    MGCR_CHECK(matrix_form || k_ri[0] != 0. || k_ri[1] != 0., MGCR_ERR_INVALID, "%s: No k value supplied for Dirac Operator!", who);
    MGCR_CHECK(n < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "%s: matrix dimensions must fit int32 per GPU (got %lld)", who, (long long)n);
    EvenOddPlan plan;
    std::vector<double> d;
    int64_t n_diag = 0;
    std::string err;
    if (!evenodd_plan_build_diag(n, rowptr, col, val_ri, parity, &plan, &d, &n_diag, &err)) {
        set_error("%s: %s", who, err.c_str());
        return MGCR_ERR_INVALID;
    }
    LOCK();
    EoState *e = new EoState();
    auto fail = [&](int rc) { eo_destroy(e); return rc; };
    e->n = n; e->ne = (int64_t)plan.even.size(); e->no = (int64_t)plan.odd.size(); e->nnz = rowptr[n];
    e->parity = plan.parity;
    const cplx k = matrix_form ? make_double2(0., 0.) : make_double2(k_ri[0], k_ri[1]);
    e->k = k;
    e->k2 = host_cmul(k, k);
    // Dirac form without a single stored diagonal entry: the operator of mgcr_eo_create, on its code path (Rule 3d)
    e->has_diag = matrix_form || n_diag > 0;
    e->matrix_form = matrix_form;
    if (e->has_diag) {
        e->c = matrix_form ? make_double2(-1., 0.) : k;
        e->c2 = host_cmul(e->c, e->c);
        e->cn = make_double2(-e->c.x, -e->c.y);
        for (int64_t r : plan.even) e->h_d_even.push_back(make_double2(d[2 * (size_t)r], d[2 * (size_t)r + 1]));
        for (int64_t r : plan.odd) e->h_d_odd.push_back(make_double2(d[2 * (size_t)r], d[2 * (size_t)r + 1]));
        const int64_t bad = diag_first_singular(e, k, matrix_form ? 1 : 0);
        if (bad >= 0) {
            set_error("%s: the diagonal of odd row %lld has no inverse (a singular diagonal block: %s = 0 or not finite)", who, (long long)bad,
                      matrix_form ? "d" : "1 - k d");
            return fail(MGCR_ERR_INVALID);
        }
    }
    int brc = eo_build_halves(e, plan, who);
    if (brc != MGCR_OK) return fail(brc);
    if (e->has_diag) {
        const size_t se = (size_t)(e->ne ? e->ne : 1), so = (size_t)(e->no ? e->no : 1);
        hipError_t rc = hipMalloc((void **)&e->dd_even, sizeof(cplx) * se);
        if (rc == hipSuccess) rc = hipMalloc((void **)&e->dd_odd, sizeof(cplx) * so);
        if (rc == hipSuccess) rc = hipMalloc((void **)&e->a_even, sizeof(cplx) * se);
        if (rc == hipSuccess) rc = hipMalloc((void **)&e->inv_a_odd, sizeof(cplx) * so);
        if (rc == hipSuccess && e->ne) rc = hipMemcpy(e->dd_even, e->h_d_even.data(), sizeof(cplx) * (size_t)e->ne, hipMemcpyHostToDevice);
        if (rc == hipSuccess && e->no) rc = hipMemcpy(e->dd_odd, e->h_d_odd.data(), sizeof(cplx) * (size_t)e->no, hipMemcpyHostToDevice);
        if (rc != hipSuccess) {
            set_error("%s: device allocation failed: %s", who, hipGetErrorString(rc));
            return fail(MGCR_ERR_ALLOC);
        }
        brc = diag_set_coefficients(e, k);
        if (brc != MGCR_OK) return fail(brc);
    }
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC_EO;
    op->dim = op->nrow = e->ne;
    op->k = e->k;
    op->eo = e;
    *out = op;
    return MGCR_OK;
}

int mgcr_eo_diag(mgcr_op_t eo, double *a_even_ri, double *inv_a_odd_ri) {
    const char *who = "mgcr_eo_diag";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(eo && eo->kind == OP_DIRAC_EO && eo->eo, MGCR_ERR_INVALID, "%s: not an even-odd preconditioned DiracOp", who);
    LOCK();
    const EoState *e = eo->eo;
    MGCR_CHECK(!e->has_block, MGCR_ERR_INVALID, "%s: the operator carries a dense block per site (mgcr_eo_create_block): mgcr_eo_block_diag downloads the blocks", who);
    MGCR_CHECK((a_even_ri || e->ne == 0) && (inv_a_odd_ri || e->no == 0), MGCR_ERR_INVALID, "%s: null argument", who);
    if (!e->has_diag) {
        for (int64_t i = 0; i < e->ne; i++) { a_even_ri[2 * i] = 1.; a_even_ri[2 * i + 1] = 0.; }
        for (int64_t i = 0; i < e->no; i++) { inv_a_odd_ri[2 * i] = 1.; inv_a_odd_ri[2 * i + 1] = 0.; }
        return MGCR_OK;
    }
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    if (e->ne) MGCR_HIP(hipMemcpy(a_even_ri, e->a_even, sizeof(cplx) * (size_t)e->ne, hipMemcpyDeviceToHost));
    if (e->no) MGCR_HIP(hipMemcpy(inv_a_odd_ri, e->inv_a_odd, sizeof(cplx) * (size_t)e->no, hipMemcpyDeviceToHost));
    return MGCR_OK;
}

}  // extern "C"
