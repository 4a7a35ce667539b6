// The low-precision GCR in EVEN-ODD form (mgcr_gcr32_create_eo): an OP_GCR32 whose matrix is the fp32 copy of the Schur complement
//     S = diag(a_e) - c^2 H_eo diag(1 / a_o) H_oe
// on the even half (gcr32_eo_plan.h has the values, include/mgcr.h the arithmetic, DESIGN.md §11 the byte model).  The inner solve is
// gcr32.hip's, on n_e elements: entry, build, update and exit are its kernels, and "the apply of this operator" is the two launches
// of this file,
//     stage 1 (odd rows)    u = H_oe r,  t = (1 / a_o) (.) u                        g32_eo_stage1_kernel<REAL, DIAG>
//     stage 2 (even rows)   v = H_eo t,  w = c2 v,  Ar = a_e (.) r - w, <Ap_j, Ar>   g32_eo_stage2_kernel<ND, REAL, DIAG>
// 4 * max_iter + 2 launches per apply.  Both stages take the apply's early returns — SkipRef, stop_u, the tolerance test on the folded
// S2 — from the same words and partials, so they end together; stage 2 alone writes stop_a, stage 1 writes t and nothing else, and
// neither reads a word its own launch writes.  No atomics, no waits, nothing exchanged inside a launch.
#include <cmath>
#include <string>

#include "evenodd_state.h"
#include "gcr32_eo_plan.h"
#include "gcr32_row_dev.h"
#include "gcr32_state.h"

namespace mgcr {

struct G32Half {   // one fp32 half on the device (owned)
    float *val = nullptr, *tail_val = nullptr;
    int32_t *col = nullptr, *tile_tail = nullptr, *tail_rows = nullptr, *tail_ptr = nullptr, *tail_col = nullptr;
    int64_t npad = 0, n_tail_rows = 0;
    int32_t W = 0;
    G32Mat mat() const { return G32Mat{val, col, npad, W, tile_tail, tail_rows, tail_ptr, tail_col, tail_val}; }
};

struct Gcr32EoState {
    Gcr32EoPlan plan;          // the host plan, slabs dropped after the upload: parity, the lists and d stay (set_k, the slot check)
    int64_t n = 0, ne = 0, no = 0, stored_bytes = 0;
    G32Half half[2];           // H_eo, H_oe
    bool has_diag = false, matrix_form = false;
    float *a_even = nullptr, *inv_a_odd = nullptr;   // c32 [n_e], [n_o]; null without a diagonal
    c32 c2 = {0.f, 0.f};
    float *t = nullptr;        // c32 [n_o]: stage 1's result
};

// ---- stage 1: t = (1 / a_o) (.) (H_oe r) over the odd rows ------------------------------------------------------------------------
template <bool REAL, bool DIAG>
__global__ void __launch_bounds__(RED_THREADS, 8)
    g32_eo_stage1_kernel(G32Mat H, const c32 *__restrict__ r, const c32 *__restrict__ inv_o, c32 *__restrict__ t, int64_t no,
                         const double *__restrict__ S2, int nblkS, double tol2, const G32Dev *__restrict__ st, int it, SKIP_ARGS) {
    SKIP_RETURN();
    __shared__ double lds[2 * 17];
    if (it > 0) {
        if (st->stop_u < it) return;
        double s2[2];
        fold_partials<2>(S2, nblkS, RED_MAX_BLOCKS, s2, lds);
        if (!(s2[1] > tol2 * s2[0])) return;   // stage 2 of this step takes the same decision and records it
    }
    const int64_t ntiles = (no + G32_TILE - 1) / G32_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * G32_TILE + threadIdx.x;
        if (row < no) {
            float ux, uy;
            g32_row_sum<REAL>(H, r, tile, row, ux, uy);
            c32 tv = make_float2(ux, uy);
            if (DIAG) {
                const c32 s = inv_o[row];
                tv = make_float2(s.x * ux - s.y * uy, s.x * uy + s.y * ux);
            }
            t[row] = tv;
        }
    }
}

// ---- stage 2: Ar = a_e (.) r - c2 (H_eo t) over the even rows; it == 0: the bare apply of mgcr_gcr32_apply_matrix ------------------
template <int ND, bool REAL, bool DIAG>
__global__ void __launch_bounds__(RED_THREADS, (ND <= 5 ? 8 : 4))
    g32_eo_stage2_kernel(G32Mat H, const c32 *__restrict__ t, const c32 *__restrict__ r, const c32 *__restrict__ a_e, c32 *__restrict__ ar,
                         const c32 *__restrict__ aps, int64_t nv, int64_t ne, c32 c2, const double *__restrict__ S2, int nblkS, double tol2,
                         G32Dev *__restrict__ st, int it, double *__restrict__ partsB, SKIP_ARGS) {
    SKIP_RETURN();
    __shared__ double lds[(ND ? 2 * ND : 2) * 17];
    if (it > 0) {
        if (st->stop_u < it) return;
        double s2[2];
        fold_partials<2>(S2, nblkS, RED_MAX_BLOCKS, s2, lds);
        if (!(s2[1] > tol2 * s2[0])) {   // |r|^2 <= tol^2 |f|^2, f = 0 included: the solve is over with what x holds
            if (blockIdx.x == 0 && threadIdx.x == 0) st->stop_a = it - 1;
            return;
        }
    }
    double acc[ND ? 2 * ND : 1] = {};
    const int64_t ntiles = (ne + G32_TILE - 1) / G32_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * G32_TILE + threadIdx.x;
        if (row < ne) {
            float vx, vy;
            g32_row_sum<REAL>(H, t, tile, row, vx, vy);
            const float wx = c2.x * vx - c2.y * vy, wy = c2.x * vy + c2.y * vx;
            const c32 own = r[row];
            c32 y;
            if (DIAG) {
                const c32 a = a_e[row];
                const float px = a.x * own.x - a.y * own.y, py = a.x * own.y + a.y * own.x;
                y = make_float2(px - wx, py - wy);
            } else {
                y = make_float2(own.x - wx, own.y - wy);
            }
            ar[row] = y;
            if constexpr (ND > 0) {
                const double yx = (double)y.x, yy = (double)y.y;
#pragma unroll
                for (int j = 0; j < ND; j++) {   // <Ap_j, Ar> = sum conj(Ap_j) Ar
                    const c32 a = aps[(int64_t)j * nv + row];
                    const double ax = (double)a.x, ay = (double)a.y;
                    acc[2 * j] += ax * yx + ay * yy;
                    acc[2 * j + 1] += ax * yy - ay * yx;
                }
            }
        }
    }
    if constexpr (ND > 0) block_sums_to_slab<2 * ND>(acc, lds, partsB, blockIdx.x);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static void g32_half_free(G32Half *h) {
    hipFree(h->val); hipFree(h->tail_val); hipFree(h->col); hipFree(h->tile_tail); hipFree(h->tail_rows); hipFree(h->tail_ptr); hipFree(h->tail_col);
}
void gcr32_eo_destroy(Gcr32EoState *e) {
    if (!e) return;
    g32_half_free(&e->half[0]);
    g32_half_free(&e->half[1]);
    hipFree(e->a_even); hipFree(e->inv_a_odd); hipFree(e->t);
    delete e;
}

static int g32_half_upload(G32Half *h, const Gcr32Plan &p) {
    h->npad = p.npad; h->W = p.W; h->n_tail_rows = (int64_t)p.tail_rows.size();
    MGCR_TRY(g32_upload(&h->val, p.ell_val));
    MGCR_TRY(g32_upload(&h->col, p.ell_col));
    MGCR_TRY(g32_upload(&h->tile_tail, p.tile_tail));
    MGCR_TRY(g32_upload(&h->tail_rows, p.tail_rows));
    MGCR_TRY(g32_upload(&h->tail_ptr, p.tail_ptr));
    MGCR_TRY(g32_upload(&h->tail_col, p.tail_col));
    return g32_upload(&h->tail_val, p.tail_val);
}

int gcr32_eo_launch_apply(Gcr32State *g, int nd, int it, SkipRef sk) {
    Gcr32EoState *e = g->eo;
    const int gs = red_grid(g->n >> 1);
    const double tol2 = g->tol * g->tol;
    const c32 *r = (const c32 *)g->r, *t = (const c32 *)e->t;
    return dispatch_bool(g->real, [&](auto real) {
        return dispatch_bool(e->has_diag, [&](auto diag) {
            constexpr bool REAL = decltype(real)::value, DIAG = decltype(diag)::value;
            if (e->no > 0)
                MGCR_TRY(launch(g32_eo_stage1_kernel<REAL, DIAG>, red_grid(e->no), RED_THREADS, 0, e->half[1].mat(), r, (const c32 *)e->inv_a_odd,
                                (c32 *)e->t, e->no, (const double *)g->S2, gs, tol2, (const G32Dev *)g->st, it, sk.p, sk.it));
            return dispatch_nd<0, GCR32_MAX_RESTART - 1>(nd, [&](auto ndc) {
                return launch(g32_eo_stage2_kernel<decltype(ndc)::value, REAL, DIAG>, red_grid(e->ne), RED_THREADS, 0, e->half[0].mat(), t, r,
                              (const c32 *)e->a_even, (c32 *)g->ar, (const c32 *)g->aps, g->nv, e->ne, e->c2, (const double *)g->S2, gs, tol2, g->st, it,
                              g->partsB, sk.p, sk.it);
            });
        });
    });
}

// a_e, 1 / a_o (in stream order behind what is enqueued) and c2 (a kernel argument) at k; refused: nothing is touched
static int g32_eo_set_coefficients(Gcr32EoState *e, const double *k_ri, const char *who) {
    Gcr32EoCoef co;
    std::string err;
    if (!gcr32_eo_coefficients(e->plan, k_ri, &co, &err)) {
        set_error("%s: %s", who, err.c_str());
        return MGCR_ERR_INVALID;
    }
    if (e->has_diag) {
        hipStream_t s = ctx().stream;
        if (e->ne) MGCR_HIP(hipMemcpyAsync(e->a_even, co.a_even.data(), sizeof(float) * co.a_even.size(), hipMemcpyHostToDevice, s));
        if (e->no) MGCR_HIP(hipMemcpyAsync(e->inv_a_odd, co.inv_a_odd.data(), sizeof(float) * co.inv_a_odd.size(), hipMemcpyHostToDevice, s));
        MGCR_HIP(hipStreamSynchronize(s));   // (the host copies go away with this frame)
    }
    e->c2 = make_float2(co.c2[0], co.c2[1]);
    return MGCR_OK;
}

int gcr32_eo_set_k(Gcr32State *g, const double k_ri[2], const char *who) { return g32_eo_set_coefficients(g->eo, k_ri, who); }

int gcr32_eo_slot_check(const Gcr32EoState *e, const Op *A) {
    if (A->kind != OP_DIRAC_EO || !A->eo) return MGCR_OK;
    const EoState *o = A->eo;
    MGCR_CHECK(!o->has_block, MGCR_ERR_UNSUPPORTED,
               "a low-precision GCR in even-odd form covers the scalar forms only: the operator of the solve carries a dense block per site");
    MGCR_CHECK(o->n == e->n && o->parity == e->plan.eo.parity, MGCR_ERR_INVALID,
               "the low-precision GCR in even-odd form and the even-odd operator of the solve differ in their rows or in their colouring "
               "(%lld and %lld rows): both must be made from the same matrix with the same parity", (long long)e->n, (long long)o->n);
    return MGCR_OK;
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)
#define G32EO_CHECK(op, who) \
    MGCR_CHECK((op) && (op)->kind == OP_GCR32 && (op)->g32 && (op)->g32->eo, MGCR_ERR_INVALID, "%s: not a low-precision GCR in even-odd form", who)

extern "C" {

int mgcr_gcr32_create_eo(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity, const double *k_ri,
                         const mgcr_gcr_param *inner, mgcr_op_t *out) {
    const char *who = "mgcr_gcr32_create_eo";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && inner && n >= 0, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_TRY(g32_check_param(inner, who));
    const bool matrix_form = k_ri == nullptr;
    c32 k32 = make_float2(0.f, 0.f);
    if (k_ri) MGCR_TRY(g32_check_k(k_ri, &k32, who));
    MGCR_CHECK(n < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "%s: matrix dimensions must fit int32 per GPU (got %lld)", who, (long long)n);
    Gcr32EoState *e = new Gcr32EoState();
    Gcr32State *g = new Gcr32State();
    g->eo = e;
    auto fail = [&](int rc) { gcr32_destroy(g); return rc; };
    std::string err;
    if (!gcr32_eo_plan_build(n, rowptr, col, val_ri, parity, matrix_form, G32_TILE, &e->plan, &err)) {
        set_error("%s: %s", who, err.c_str());
        return fail(MGCR_ERR_INVALID);
    }
    LOCK();
    const Gcr32EoPlan &p = e->plan;
    e->n = n; e->ne = (int64_t)p.eo.even.size(); e->no = (int64_t)p.eo.odd.size(); e->stored_bytes = p.stored_bytes();
    e->has_diag = p.has_diag; e->matrix_form = matrix_form;
    g->n = e->ne; g->nv = (e->ne + 3) / 4 * 4; g->nnz = p.nnz; g->stored_bytes = e->stored_bytes;
    g->real = p.real_slab; g->dirac = !matrix_form;
    if (k_ri) { g->k_ri[0] = k_ri[0]; g->k_ri[1] = k_ri[1]; g->k32 = k32; }
    g->restart = inner->restart; g->max_iter = inner->max_iter; g->tol = inner->tol;
    int rc = g32_half_upload(&e->half[0], p.half[0]);
    if (rc == MGCR_OK) rc = g32_half_upload(&e->half[1], p.half[1]);
    if (rc == MGCR_OK) rc = g32_alloc(&e->t, (size_t)2 * (size_t)e->no);
    if (rc == MGCR_OK && e->has_diag) rc = g32_alloc(&e->a_even, (size_t)2 * (size_t)e->ne);
    if (rc == MGCR_OK && e->has_diag) rc = g32_alloc(&e->inv_a_odd, (size_t)2 * (size_t)e->no);
    if (rc == MGCR_OK) rc = g32_eo_set_coefficients(e, k_ri, who);
    if (rc == MGCR_OK) rc = g32_alloc_iteration(g);
    if (rc != MGCR_OK) return fail(rc);
    for (int h = 0; h < 2; h++) {   // the slabs live on the device now; the lists, the parity and d stay
        Gcr32Plan &hp = e->plan.half[h];
        std::vector<float>().swap(hp.ell_val);
        std::vector<int32_t>().swap(hp.ell_col);
        std::vector<float>().swap(hp.tail_val);
        std::vector<int32_t>().swap(hp.tail_col);
    }
    e->plan.eo.eo = HalfCsr();
    e->plan.eo.oe = HalfCsr();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_GCR32;
    op->dim = op->nrow = e->ne;
    op->g32 = g;
    *out = op;
    return MGCR_OK;
}

int mgcr_gcr32_eo_info(mgcr_op_t op, int64_t *n, int64_t *n_even, int64_t *n_odd, int32_t *width_eo, int32_t *width_oe, int64_t *tail_rows_eo,
                       int64_t *tail_rows_oe, int32_t *real_slab, int32_t *has_diag, int64_t *stored_bytes) {
    G32EO_CHECK(op, "mgcr_gcr32_eo_info");
    const Gcr32EoState *e = op->g32->eo;
    if (n) *n = e->n;
    if (n_even) *n_even = e->ne;
    if (n_odd) *n_odd = e->no;
    if (width_eo) *width_eo = e->half[0].W;
    if (width_oe) *width_oe = e->half[1].W;
    if (tail_rows_eo) *tail_rows_eo = e->half[0].n_tail_rows;
    if (tail_rows_oe) *tail_rows_oe = e->half[1].n_tail_rows;
    if (real_slab) *real_slab = op->g32->real ? 1 : 0;
    if (has_diag) *has_diag = e->has_diag ? 1 : 0;
    if (stored_bytes) *stored_bytes = e->stored_bytes;
    return MGCR_OK;
}

int mgcr_gcr32_eo_diag(mgcr_op_t op, float *a_even_ri, float *inv_a_odd_ri) {
    const char *who = "mgcr_gcr32_eo_diag";
    MGCR_TRY(require_ctx());
    G32EO_CHECK(op, who);
    LOCK();
    const Gcr32EoState *e = op->g32->eo;
    MGCR_CHECK((a_even_ri || e->ne == 0) && (inv_a_odd_ri || e->no == 0), MGCR_ERR_INVALID, "%s: null argument", who);
    if (!e->has_diag) {
        for (int64_t i = 0; i < e->ne; i++) { a_even_ri[2 * i] = 1.f; a_even_ri[2 * i + 1] = 0.f; }
        for (int64_t i = 0; i < e->no; i++) { inv_a_odd_ri[2 * i] = 1.f; inv_a_odd_ri[2 * i + 1] = 0.f; }
        return MGCR_OK;
    }
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    if (e->ne) MGCR_HIP(hipMemcpy(a_even_ri, e->a_even, sizeof(float) * 2 * (size_t)e->ne, hipMemcpyDeviceToHost));
    if (e->no) MGCR_HIP(hipMemcpy(inv_a_odd_ri, e->inv_a_odd, sizeof(float) * 2 * (size_t)e->no, hipMemcpyDeviceToHost));
    return MGCR_OK;
}

}  // extern "C"
