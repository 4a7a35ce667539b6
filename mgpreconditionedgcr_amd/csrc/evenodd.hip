// Even-odd (red-black) preconditioned DiracOp, OP_DIRAC_EO.  D is a pure hopping matrix: no diagonal, even rows coupled to odd rows
// only (evenodd_plan.h finds and checks the colouring).  A = 1 - k D then reduces to the Schur complement on the even half,
//     S x_e = bhat_e,   S = 1 - k^2 D_eo D_oe,   bhat_e = b_e + k D_eo b_o,   x_o = b_o + k D_oe x_e,
// and the operator this file makes IS S: an Operator on Fields of n_e entries that GCR solves like any other.  An apply of S reads
// every stored entry of D once, like the full apply; every Krylov vector is half as long.
//
// Both halves are ordinary Sparse operators (csr_build_device chooses their storage), the apply is two csr_apply launches
//     t = D_oe x;   y = x - k2 (D_eo t)      (k2 = k k, formed once on the host, un-fused)
// and inside a GCR step the second one is schur_step_apply_kernel below: stage 2 together with the step's beta dot products, the
// counterpart of gcr_fused.hip's step_apply_kernel — same row map, same per-thread accumulation order, same block sum and partial
// layout, so the folds that follow consume its partials unchanged, and y and the partials have the bits of the plain stage 2
// followed by multidot_kernel (tests/test_gpu_evenodd.py, Rule 2 of include/mgcr.h).
#include <algorithm>
#include <string>

#include "internal.h"
#include "reduce.h"
#include "spmv_dev.h"
#include "gcr_dev.h"
#include "evenodd_plan.h"
#include "evenodd_state.h"

namespace mgcr {

void eo_destroy(EoState *e) {
    if (!e) return;
    for (mgcr_op_s *h : e->half)
        if (h) { csr_free(&h->csr); delete h; }
    hipFree(e->d_even); hipFree(e->d_odd); hipFree(e->t);
    eo_diag_destroy(e);
    eo_block_destroy(e);
    gcr_state_destroy(e->solver);
    for (cplx *w : e->work) hipFree(w);
    delete e;
}
int64_t eo_nnz(const EoState *e) { return e ? e->nnz : -1; }
static int64_t g_schur_fused_steps = 0;
int64_t eo_fused_step_count() { return g_schur_fused_steps; }

// full[list[i]] <-> half[i]; either half may be absent
__global__ void __launch_bounds__(RED_THREADS) eo_split_kernel(const cplx *__restrict__ full, cplx *__restrict__ even, cplx *__restrict__ odd,
                                                               const int32_t *__restrict__ ev, const int32_t *__restrict__ od, int64_t ne,
                                                               int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) {
            if (even) even[i] = full[ev[i]];
        } else if (odd) {
            odd[i - ne] = full[od[i - ne]];
        }
    }
}
__global__ void __launch_bounds__(RED_THREADS) eo_merge_kernel(cplx *__restrict__ full, const cplx *__restrict__ even, const cplx *__restrict__ odd,
                                                               const int32_t *__restrict__ ev, const int32_t *__restrict__ od, int64_t ne,
                                                               int64_t no) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + no; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) full[ev[i]] = even[i];
        else full[od[i - ne]] = odd[i - ne];
    }
}
int eo_split(const EoState *e, const cplx *full, cplx *even, cplx *odd) {
    if (e->n == 0) return MGCR_OK;
    return launch(eo_split_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, full, even, odd, (const int32_t *)e->d_even, (const int32_t *)e->d_odd,
                  e->ne, e->no);
}
int eo_merge(const EoState *e, cplx *full, const cplx *even, const cplx *odd) {
    if (e->n == 0) return MGCR_OK;
    return launch(eo_merge_kernel, (unsigned)red_grid(e->n), RED_THREADS, 0, full, even, odd, (const int32_t *)e->d_even, (const int32_t *)e->d_odd,
                  e->ne, e->no);
}

int eo_work(EoState *e, EoState::Work which, cplx **out) {
    if (!e->work[which]) {
        const int64_t len = (which == EoState::W_BO || which == EoState::W_XO || which == EoState::W_UO) ? e->no : e->ne;
        hipError_t rc = hipMalloc((void **)&e->work[which], sizeof(cplx) * (size_t)(len ? len : 1));
        MGCR_CHECK(rc == hipSuccess, MGCR_ERR_ALLOC, "even-odd DiracOp: hipMalloc of a work Field failed: %s", hipGetErrorString(rc));
    }
    *out = e->work[which];
    return MGCR_OK;
}

// y = w - c u, skip-aware like the operator applies
__global__ void __launch_bounds__(RED_THREADS) eo_sub_scaled_kernel(cplx *__restrict__ y, const cplx *__restrict__ w, cplx c, const cplx *__restrict__ u,
                                                                    int64_t n, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = csub(w[i], cmul(c, u[i]));
}

// y = w - c (H x) for half H (0: D_eo, 1: D_oe) with the bits of "u = H x, then y = w - c u" (Rule 1 of include/mgcr.h).  The SpMV's
// shifted epilogue forms exactly that — unless the half keeps long rows in a CSR tail, whose kernels subtract their part of the row in a
// second step ((w - c s_slab) - c s_tail): such a half is multiplied unshifted into a work Field and subtracted in a launch of its own.
int eo_shift_apply(EoState *e, int h, const cplx *x, cplx *y, cplx c, const cplx *w) {
    const CsrDev &A = e->half[h]->csr;
    if (A.nrow == 0) return MGCR_OK;
    if (A.n_tail_rows == 0) return csr_apply(A, x, y, true, c, nullptr, w);
    cplx *u;
    MGCR_TRY(eo_work(e, h == 0 ? EoState::W_UE : EoState::W_UO, &u));
    MGCR_TRY(csr_apply(A, x, u, false, make_double2(0., 0.)));
    const SkipRef sk = get_apply_skip();
    return launch(eo_sub_scaled_kernel, (unsigned)red_grid(A.nrow), RED_THREADS, 0, y, w, c, (const cplx *)u, A.nrow, sk.p, sk.it);
}

int eo_apply(Op *op, const cplx *x, cplx *y, int64_t n) {
    EoState *e = op->eo;
    MGCR_CHECK(e && n == e->ne, MGCR_ERR_INVALID, "even-odd DiracOp: the Field must have the %lld entries of the even half", (long long)(e ? e->ne : 0));
    if (e->has_diag) return eo_diag_apply(e, x, y);   // a site diagonal: evenodd_diag.hip
    if (e->has_block) return eo_block_apply(e, x, y);   // a dense block per site: evenodd_block.hip
    MGCR_CHECK(e->k.x != 0. || e->k.y != 0., MGCR_ERR_INVALID, "No k value supplied for Dirac Operator!");
    MGCR_TRY(csr_apply(e->half[1]->csr, x, e->t, false, make_double2(0., 0.)));
    return eo_shift_apply(e, 0, e->t, y, e->k2, x);
}

// ---- stage 2 of a GCR step with the beta dot products -------------------------------------------------------------------------
struct SchurDots {
    const cplx *v[FND];
};

// y = w - k2 (D_eo t) and the partial sums of <y, Ap_j>, j < NDT: step_apply_kernel (gcr_fused.hip) with the gathered operand t
// apart from the row's own term w.  Plain row map (band 0).  The direction streams are requested behind the row product for the
// reason given there: gathers and streams never hold registers together.
// MODE 0 slab, 1 / 2 dictionary, 3 stencil view (WT = 7 or 9 slots).  The rare-tail layout of the stencil view (MODE 4 there — the halo
// columns of a distributed row block) has no instantiation: under the 8-wave bound it needs 20 B of scratch at 5 directions, and
// distributed use is out of scope; such a D_eo takes the plain stage 2 and multidot_kernel (eo_schur_fusable).
template <int MODE, int WT, int NDT>
__global__ void __launch_bounds__(RED_THREADS, ((MODE == 1 || (MODE == 3 && WT <= 7)) && NDT <= 5 ? 8 : 4))
    schur_step_apply_kernel(RowMat m, const cplx *__restrict__ t, const cplx *__restrict__ w, cplx *__restrict__ y, SchurDots d, int64_t n,
                            int nlogical, RowMap rm, double *__restrict__ parts, const int *__restrict__ skip, int skip_it) {
    __shared__ double lds[2 * NDT * 17];
    extern __shared__ __attribute__((aligned(16))) unsigned char schur_smem[];
    if (skip && skip[0] < skip[1] + skip_it) return;
    const int lb = logical_workgroup(rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= nlogical) return;
    const int32_t W = WT ? WT : m.W;
    int64_t first, last, step;
    row_range(rm, lb, nlogical, n, &first, &last, &step);
    // (rows fit 31 bits, csr_build_device, and a step is at most 2^19 rows: the row number is kept in ONE register — worth 2 to 6 VGPRs,
    // what the 5-direction dictionary form needs to stay within 64 without scratch)
    uint32_t i = (uint32_t)first;
    const uint32_t end = (uint32_t)last, stride = (uint32_t)step;
    int32_t t0 = 0;
    if ((MODE == 1 || MODE == 2) && i < end) t0 = (int32_t)__builtin_nontemporal_load(m.pid + i) * W;
    PatLds pl{nullptr, nullptr, nullptr};
    if (MODE == 1) pl = stage_patterns(m, schur_smem);
    double v[2 * NDT];
#pragma unroll
    for (int j = 0; j < 2 * NDT; j++) v[j] = 0.;
    for (; i < end; i += stride) {
        int32_t t0_next = 0;
        if ((MODE == 1 || MODE == 2) && i + stride < end) t0_next = (int32_t)__builtin_nontemporal_load(m.pid + i + stride) * W;
        const cplx sum = fused_row_product<MODE, WT>(m, i, t0, pl, [&](int32_t j) -> cplx { return t[j]; });
        const cplx yi = csub(w[i], cmul(m.k, sum));
        y[i] = yi;
        __builtin_amdgcn_sched_barrier(0);
        cplx b[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) b[j] = ld_stream<true>(d.v[j] + i);
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            cplx u = cconj_mul(yi, b[j]);
            v[2 * j] += u.x;
            v[2 * j + 1] += u.y;
        }
        t0 = t0_next;
    }
    const double mine = block_sum_owner<2 * NDT>(v, lds);
    if (threadIdx.x < 2 * NDT) parts[(size_t)threadIdx.x * RED_MAX_BLOCKS + lb] = mine;
}

bool eo_schur_fusable(const Op *op) {
    if (!op || op->kind != OP_DIRAC_EO || !op->eo || !fuse_enabled()) return false;
    if (op->eo->has_diag) return eo_diag_schur_fusable(op->eo);
    if (op->eo->has_block) return eo_block_schur_fusable(op->eo);
    const CsrDev &A = op->eo->half[0]->csr;
    if (A.pat_mode == 1 && (int64_t)A.npat * A.W * 20 > 48 * 1024) return false;   // the pattern table must fit LDS
    if (csr_stencil_active(A) && A.sten_rare) return false;                        // (no rare-tail form: see the kernel)
    return A.L == 1 && A.n_tail_rows == 0 && A.nrow >= 1 && A.W >= 1;
}

int eo_schur_step(Op *op, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm) {
    EoState *e = op->eo;
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "SpMV cannot run in place");
    MGCR_CHECK(nd >= 1 && nd <= FND, MGCR_ERR_INVALID, "eo_schur_step: 1..%d vectors", FND);
    MGCR_CHECK(rm.band == 0, MGCR_ERR_INVALID, "eo_schur_step: plain row map only");
    if (e->has_diag) return eo_diag_schur_step(e, x, y, vecs, nd, parts, rm);
    if (e->has_block) return eo_block_schur_step(e, x, y, vecs, nd, parts, rm);
    MGCR_CHECK(e->k.x != 0. || e->k.y != 0., MGCR_ERR_INVALID, "No k value supplied for Dirac Operator!");
    MGCR_TRY(csr_apply(e->half[1]->csr, x, e->t, false, make_double2(0., 0.)));
    const CsrDev &A = e->half[0]->csr;
    const RowMat m = row_mat(A, true, e->k2);
    SchurDots d;
    for (int j = 0; j < FND; j++) d.v[j] = vecs[j < nd ? j : 0];
    const int g = red_grid(A.nrow);
    const unsigned grid = fused_grid(g);
    const SkipRef sk = get_apply_skip();
    MGCR_CHECK(eo_schur_fusable(op), MGCR_ERR_INVALID, "eo_schur_step: D_eo is not stored in a form the fused stage exists for");
    // the (MODE, WT) pairs of fused_form's plain forms: stencil view of 7 / 9 slots, dictionary, slab; width 7 compiled in
    const bool sten = csr_stencil_active(A);
    const int mode = sten ? 3 : (A.pat_mode == 1 || A.pat_mode == 2 ? A.pat_mode : 0);
    const int wt = sten ? (sten_slots(A) != 7 ? 9 : 7) : (A.W == 7 ? 7 : 0);
    const size_t lds = sten ? 0 : row_mat_lds_bytes(A);
    const cplx *t = e->t;
    g_schur_fused_steps++;
    return dispatch_value<3, 1, 2, 0>(mode, [&](auto MODE) -> int {
        return dispatch_value<9, 7, 0>(wt, [&](auto WTT) -> int {
            constexpr int M = decltype(MODE)::value, WW = decltype(WTT)::value;
            if constexpr (M == 3 ? WW != 0 : WW != 9) {
                return dispatch_nd<1, FND>(nd, [&](auto NDT) -> int {
                    return launch(schur_step_apply_kernel<M, WW, decltype(NDT)::value>, grid, RED_THREADS, lds, m, t, x, y, d, A.nrow, g, rm, parts,
                                  sk.p, sk.it);
                });
            } else {
                set_error("even-odd GCR step: no kernel of this form");
                return MGCR_ERR_INVALID;
            }
        });
    });
}

// the two halves as Sparse operators, the index lists and t on the device; e->ne / e->no must be set.  On failure the caller destroys e.
int eo_build_halves(EoState *e, const EvenOddPlan &plan, const char *who) {
    const HalfCsr *hc[2] = {&plan.eo, &plan.oe};
    for (int h = 0; h < 2; h++) {
        mgcr_op_s *op = new mgcr_op_s();
        op->kind = OP_CSR;
        op->dim = hc[h]->ncol;
        op->nrow = hc[h]->nrow;
        e->half[h] = op;
        MGCR_TRY(csr_build_device(hc[h]->nrow, hc[h]->ncol, hc[h]->rowptr.data(), hc[h]->col.data(), hc[h]->val_ri.data(), &op->csr));
    }
    std::vector<int32_t> ev(plan.even.begin(), plan.even.end()), od(plan.odd.begin(), plan.odd.end());
    hipError_t rc = hipMalloc((void **)&e->d_even, sizeof(int32_t) * (ev.size() ? ev.size() : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->d_odd, sizeof(int32_t) * (od.size() ? od.size() : 1));
    if (rc == hipSuccess) rc = hipMalloc((void **)&e->t, sizeof(cplx) * (size_t)(e->no ? e->no : 1));
    if (rc == hipSuccess && !ev.empty()) rc = hipMemcpy(e->d_even, ev.data(), sizeof(int32_t) * ev.size(), hipMemcpyHostToDevice);
    if (rc == hipSuccess && !od.empty()) rc = hipMemcpy(e->d_odd, od.data(), sizeof(int32_t) * od.size(), hipMemcpyHostToDevice);
    MGCR_CHECK(rc == hipSuccess, MGCR_ERR_ALLOC, "%s: device allocation failed: %s", who, hipGetErrorString(rc));
    return MGCR_OK;
}

// bhat = b_e - (-k) (D_eo b_o); the halves of b stay in W_BE, W_BO
static int eo_prepare(EoState *e, const cplx *b_full, cplx *bhat) {
    if (e->has_diag) return eo_diag_prepare(e, b_full, bhat);
    if (e->has_block) return eo_block_prepare(e, b_full, bhat);
    cplx *be, *bo;
    MGCR_TRY(eo_work(e, EoState::W_BE, &be));
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    MGCR_TRY(eo_split(e, b_full, be, bo));
    return eo_shift_apply(e, 0, bo, bhat, make_double2(-e->k.x, -e->k.y), be);
}
// x_o = b_o - (-k) (D_oe x_e), then x_full = merge(x_e, x_o)
static int eo_reconstruct(EoState *e, const cplx *b_full, const cplx *xe, cplx *x_full) {
    if (e->has_diag) return eo_diag_reconstruct(e, b_full, xe, x_full);
    if (e->has_block) return eo_block_reconstruct(e, b_full, xe, x_full);
    cplx *bo, *xo;
    MGCR_TRY(eo_work(e, EoState::W_BO, &bo));
    MGCR_TRY(eo_work(e, EoState::W_XO, &xo));
    MGCR_TRY(eo_split(e, b_full, nullptr, bo));
    MGCR_TRY(eo_shift_apply(e, 1, xe, xo, make_double2(-e->k.x, -e->k.y), bo));
    return eo_merge(e, x_full, xe, xo);
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)
#define EO_CHECK(op, who) MGCR_CHECK((op) && (op)->kind == OP_DIRAC_EO && (op)->eo, MGCR_ERR_INVALID, "%s: not an even-odd preconditioned DiracOp", who)
#define EO_LEN(v, len, who, what)                                                                                                     \
    MGCR_CHECK((v)->n == (len), MGCR_ERR_INVALID, "%s: the %s Field has %lld entries, %lld are needed", who, what, (long long)(v)->n, (long long)(len))

extern "C" {

int mgcr_eo_create(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity, const double k_ri[2],
                   mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && k_ri && n >= 0, MGCR_ERR_INVALID, "mgcr_eo_create: null argument");
    MGCR_CHECK(k_ri[0] != 0. || k_ri[1] != 0., MGCR_ERR_INVALID, "mgcr_eo_create: No k value supplied for Dirac Operator!");
    MGCR_CHECK(n < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "mgcr_eo_create: matrix dimensions must fit int32 per GPU (got %lld)", (long long)n);
    EvenOddPlan plan;
    std::string err;
    if (!evenodd_plan_build(n, rowptr, col, val_ri, parity, &plan, &err)) {
        set_error("mgcr_eo_create: %s", err.c_str());
        return MGCR_ERR_INVALID;
    }
    LOCK();
    EoState *e = new EoState();
    e->n = n; e->ne = (int64_t)plan.even.size(); e->no = (int64_t)plan.odd.size(); e->nnz = rowptr[n];
    e->parity = plan.parity;
    e->k = make_double2(k_ri[0], k_ri[1]);
    e->k2 = host_cmul(e->k, e->k);
    int brc = eo_build_halves(e, plan, "mgcr_eo_create");
    if (brc != MGCR_OK) { eo_destroy(e); return brc; }
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC_EO;
    op->dim = op->nrow = e->ne;
    op->k = e->k;
    op->eo = e;
    *out = op;
    return MGCR_OK;
}

// The values travel in the kernel arguments of every launch: what is already enqueued keeps the old ones.
int mgcr_eo_set_k(mgcr_op_t eo, const double k_ri[2]) {
    EO_CHECK(eo, "mgcr_eo_set_k");
    MGCR_CHECK(k_ri, MGCR_ERR_INVALID, "mgcr_eo_set_k: null argument");
    MGCR_CHECK(k_ri[0] != 0. || k_ri[1] != 0., MGCR_ERR_INVALID, "mgcr_eo_set_k: No k value supplied for Dirac Operator!");
    LOCK();
    if (eo->eo->has_diag) return eo_diag_set_k(eo, make_double2(k_ri[0], k_ri[1]));
    if (eo->eo->has_block) return eo_block_set_k(eo, make_double2(k_ri[0], k_ri[1]));
    eo->eo->k = eo->k = make_double2(k_ri[0], k_ri[1]);
    eo->eo->k2 = host_cmul(eo->k, eo->k);
    return MGCR_OK;
}

int mgcr_eo_info(mgcr_op_t eo, int64_t *n, int64_t *n_even, int64_t *n_odd) {
    EO_CHECK(eo, "mgcr_eo_info");
    if (n) *n = eo->eo->n;
    if (n_even) *n_even = eo->eo->ne;
    if (n_odd) *n_odd = eo->eo->no;
    return MGCR_OK;
}

int mgcr_eo_parity(mgcr_op_t eo, int8_t *parity) {
    EO_CHECK(eo, "mgcr_eo_parity");
    MGCR_CHECK(parity || eo->eo->n == 0, MGCR_ERR_INVALID, "mgcr_eo_parity: null argument");
    std::copy(eo->eo->parity.begin(), eo->eo->parity.end(), parity);
    return MGCR_OK;
}

int mgcr_eo_half_op(mgcr_op_t eo, int32_t which, mgcr_op_t *borrowed) {
    EO_CHECK(eo, "mgcr_eo_half_op");
    MGCR_CHECK(borrowed && (which == 0 || which == 1), MGCR_ERR_INVALID, "mgcr_eo_half_op: which = %d, 0 (D_eo) or 1 (D_oe)", (int)which);
    *borrowed = eo->eo->half[which];
    return MGCR_OK;
}

int mgcr_eo_split(mgcr_op_t eo, mgcr_vec_t full, mgcr_vec_t even, mgcr_vec_t odd) {
    const char *who = "mgcr_eo_split";
    MGCR_TRY(require_ctx());
    EO_CHECK(eo, who);
    MGCR_CHECK(full && even && odd, MGCR_ERR_INVALID, "%s: null argument", who);
    EO_LEN(full, eo->eo->n, who, "full");
    EO_LEN(even, eo->eo->ne, who, "even");
    EO_LEN(odd, eo->eo->no, who, "odd");
    MGCR_CHECK(full != even && full != odd && even != odd, MGCR_ERR_INVALID, "%s: the three Fields must be different", who);
    LOCK();
    return eo_split(eo->eo, full->d, even->w(), odd->w());
}

int mgcr_eo_merge(mgcr_op_t eo, mgcr_vec_t even, mgcr_vec_t odd, mgcr_vec_t full) {
    const char *who = "mgcr_eo_merge";
    MGCR_TRY(require_ctx());
    EO_CHECK(eo, who);
    MGCR_CHECK(full && even && odd, MGCR_ERR_INVALID, "%s: null argument", who);
    EO_LEN(full, eo->eo->n, who, "full");
    EO_LEN(even, eo->eo->ne, who, "even");
    EO_LEN(odd, eo->eo->no, who, "odd");
    MGCR_CHECK(full != even && full != odd && even != odd, MGCR_ERR_INVALID, "%s: the three Fields must be different", who);
    LOCK();
    return eo_merge(eo->eo, full->w(), even->d, odd->d);
}

int mgcr_eo_prepare(mgcr_op_t eo, mgcr_vec_t b_full, mgcr_vec_t bhat_even) {
    const char *who = "mgcr_eo_prepare";
    MGCR_TRY(require_ctx());
    EO_CHECK(eo, who);
    MGCR_CHECK(b_full && bhat_even, MGCR_ERR_INVALID, "%s: null argument", who);
    EO_LEN(b_full, eo->eo->n, who, "full");
    EO_LEN(bhat_even, eo->eo->ne, who, "even");
    MGCR_CHECK(b_full != bhat_even, MGCR_ERR_INVALID, "%s: the two Fields must be different", who);
    LOCK();
    return eo_prepare(eo->eo, b_full->d, bhat_even->w());
}

int mgcr_eo_reconstruct(mgcr_op_t eo, mgcr_vec_t b_full, mgcr_vec_t x_even, mgcr_vec_t x_full) {
    const char *who = "mgcr_eo_reconstruct";
    MGCR_TRY(require_ctx());
    EO_CHECK(eo, who);
    MGCR_CHECK(b_full && x_even && x_full, MGCR_ERR_INVALID, "%s: null argument", who);
    EO_LEN(b_full, eo->eo->n, who, "right-hand side");
    EO_LEN(x_even, eo->eo->ne, who, "even");
    EO_LEN(x_full, eo->eo->n, who, "full");
    MGCR_CHECK(b_full != x_full && x_even != x_full && b_full != x_even, MGCR_ERR_INVALID, "%s: the three Fields must be different", who);
    LOCK();
    return eo_reconstruct(eo->eo, b_full->d, x_even->d, x_full->w());
}

int mgcr_eo_solve(mgcr_op_t eo, const mgcr_gcr_param *param, mgcr_vec_t b_full, mgcr_vec_t x_full, double *hist, int32_t hist_cap,
                  int32_t *n_iter, int32_t *converged) {
    const char *who = "mgcr_eo_solve";
    MGCR_TRY(require_ctx());
    EO_CHECK(eo, who);
    MGCR_CHECK(param && b_full && x_full, MGCR_ERR_INVALID, "%s: null argument", who);
    EO_LEN(b_full, eo->eo->n, who, "right-hand side");
    EO_LEN(x_full, eo->eo->n, who, "solution");
    MGCR_CHECK(b_full != x_full && b_full->d != x_full->d, MGCR_ERR_INVALID, "rhs and x must be different Fields");
    LOCK();
    EoState *e = eo->eo;
    cplx *bhat, *xe;
    MGCR_TRY(eo_work(e, EoState::W_BHAT, &bhat));
    MGCR_TRY(eo_work(e, EoState::W_XE, &xe));
    const bool xz = x_full->zero_known;
    MGCR_TRY(eo_prepare(e, b_full->d, bhat));
    if (xz) MGCR_TRY(k_zero(xe, e->ne));
    else MGCR_TRY(eo_split(e, x_full->d, xe, nullptr));
    if (!e->solver) MGCR_TRY(gcr_state_create(eo, param, 1, &e->solver));
    else MGCR_TRY(gcr_state_set_param(e->solver, param));
    int it = 0, conv = 0;
    int rc = gcr_run(e->solver, bhat, xe, false, hist, hist_cap, &it, &conv, xz);
    if (n_iter) *n_iter = it;
    if (converged) *converged = conv;
    if (rc != MGCR_OK) return rc;
    return eo_reconstruct(e, b_full->d, xe, x_full->w());
}

}  // extern "C"
