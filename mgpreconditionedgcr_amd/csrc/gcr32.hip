// The low-precision GCR (OP_GCR32): an fp32 copy of a matrix and a restarted GCR that runs entirely in fp32 on the device, from
// x0 = 0, with no host round trip.  Applied to an fp64 Field f it returns y ~ A^-1 f: the flexible right preconditioner of an fp64
// solve (include/mgcr.h has the arithmetic, DESIGN.md §11 the byte model and the measurements).
//
//   entry    r32 = fp32(f), x32 = 0, the partials of |f|^2, the state reset
//   step k   apply<ND, REAL>   stop test on the folded |r|^2 and |f|^2; Ar = A32 r and the partials of <Ap_j, Ar>, j < ND
//            build<ND>         fold, beta_j, p and Ap into slot ND, the partials of <Ap, Ap> and <Ap, r>
//            update            fold, alpha, x, r, the partials of |r|^2, the step counter
//   exit     y = fp64(x32), |r| / |f| of the last step
// ND = (k - 1) % restart directions are stored when step k starts.  3 * max_iter + 2 launches per apply, whatever the data.
//
// Stopping.  Two kernels end the solve: the apply of step k on the tolerance (it writes G32Dev::stop_a = k - 1) and the update on
// an exactly zero <Ap, Ap> (stop_u = k - 1); both words are INT_MAX while the solve runs and a kernel of step k returns at once when
// one it reads is < k.  Every workgroup of the ending launch takes the decision from its own fold of the same partials (bit-identical
// in every workgroup, reduce.h), workgroup 0 alone writes the word, and NO kernel reads the word its own launch writes: the apply
// reads stop_u, the update stop_a, the build both (the entry kernel, which resets them, reads neither; handed the outer solve's
// stopping test — Gcr32Gate — it sets both to -1 when that solve is about to end: 0 steps, y = 0).  A later apply (update) whose word is not read therefore repeats the fold of the
// unchanged partials and ends in the same way.  Nothing is exchanged inside a launch; no atomics, no waits.
#include <cmath>

#include "gcr32_elem_dev.h"
#include "gcr32_row_dev.h"
#include "gcr32_state.h"

namespace mgcr {

// Counters on the device: {applies that ran, inner steps those enqueued}, bumped by the entry kernel's first thread — launches of one
// stream, one writer.  An apply that an outer solve silences (SkipRef) or gates (Gcr32Gate) does not count.
static long long *g_dev_counts = nullptr;
static int64_t read_count(int which) {
    if (!g_dev_counts || !ctx().ready) return 0;
    Context &c = ctx();
    std::lock_guard<std::recursive_mutex> lk(c.mtx);   // (the mailbox is the solver loop's as well)
    if (hipMemcpyAsync(c.h_mail, g_dev_counts, 2 * sizeof(long long), hipMemcpyDeviceToHost, c.stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c.stream) != hipSuccess) return -1;
    return (int64_t)((const long long *)c.h_mail)[which];
}
int64_t gcr32_apply_count() { return read_count(0); }
int64_t gcr32_step_count() { return read_count(1); }
void gcr32_release() {
    if (g_dev_counts) hipFree(g_dev_counts);
    g_dev_counts = nullptr;
}

// ---- entry: r = fp32(f), x = 0, |f|^2 (of the rounded values: what the iteration sees) -------------------------------------------
__global__ void __launch_bounds__(RED_THREADS) g32_entry_kernel(const cplx *__restrict__ f, float *__restrict__ r, float *__restrict__ x, int64_t n,
                                                                G32Dev *__restrict__ st, double *__restrict__ S2, Gcr32Gate gate,
                                                                long long *__restrict__ counts, int max_iter, SKIP_ARGS) {
    SKIP_RETURN();
    __shared__ double lds[17];
    if (st && blockIdx.x == 0) {
        // the outer solve's own test on the residual this apply was handed (close_step, gcr_dev.h: same fold, same expression, same
        // bits): when that solve is about to end here, the inner solve is cut to 0 steps — y = 0, which nobody reads
        bool gated = false;
        if (gate.partsR) {
            double rr[1];
            fold_partials<1>(gate.partsR, gate.nblk, gate.stride, rr, lds);
            gated = gcr_solve_ends(rr[0], *gate.bnorm2, *gate.tol2);
        }
        if (threadIdx.x == 0) {
            st->stop_a = st->stop_u = gated ? -1 : INT_MAX;
            st->n_iter = 0;
            st->rel = 0.;
            if (!gated && counts) { counts[0] += 1; counts[1] += max_iter; }
        }
    }
    double acc[1] = {0.};
    const int64_t npair = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx a = f[2 * i], b = f[2 * i + 1];
        const float4 v = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
        reinterpret_cast<float4 *>(r)[i] = v;
        reinterpret_cast<float4 *>(x)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc[0] += norm2d(v.x, v.y);
        acc[0] += norm2d(v.z, v.w);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
        const cplx a = f[n - 1];
        const c32 v = make_float2((float)a.x, (float)a.y);
        reinterpret_cast<c32 *>(r)[n - 1] = v;
        reinterpret_cast<c32 *>(x)[n - 1] = make_float2(0.f, 0.f);
        acc[0] += norm2d(v.x, v.y);
    }
    const double mine = block_sum_owner<1>(acc, lds);
    if (threadIdx.x == 0) { S2[blockIdx.x] = mine; S2[RED_MAX_BLOCKS + blockIdx.x] = mine; }
}

// ---- apply: Ar = A32 r, one thread per row; it == 0: the bare matrix apply of mgcr_gcr32_apply_matrix ----------------------------
template <int ND, bool REAL>
__global__ void __launch_bounds__(RED_THREADS, (ND <= 5 ? 8 : 4))
    g32_apply_kernel(G32Mat A, const c32 *__restrict__ r, c32 *__restrict__ ar, const c32 *__restrict__ aps, int64_t nv, int64_t n, int dirac,
                     c32 k32, const double *__restrict__ S2, int nblkS, double tol2, G32Dev *__restrict__ st, int it,
                     double *__restrict__ partsB, SKIP_ARGS) {
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
    const int64_t ntiles = (n + G32_TILE - 1) / G32_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * G32_TILE + threadIdx.x;
        if (row < n) {
            float sx, sy;
            g32_row_sum<REAL>(A, r, tile, row, sx, sy);
            c32 y = make_float2(sx, sy);
            if (dirac) {   // y = x - k32 s
                y = g32_dirac_shift(k32, r[row], sx, sy);
            }
            ar[row] = y;
            if constexpr (ND > 0) {
                const double yx = (double)y.x, yy = (double)y.y;
#pragma unroll
                for (int j = 0; j < ND; j++) {   // <Ap_j, Ar> = sum conj(Ap_j) Ar
                    const c32 a = aps[(int64_t)j * nv + row];
                    g32_beta_dot(a.x, a.y, yx, yy, acc[2 * j], acc[2 * j + 1]);
                }
            }
        }
    }
    if constexpr (ND > 0) block_sums_to_slab<2 * ND>(acc, lds, partsB, blockIdx.x);
}

// ---- build: beta_j, p = r - sum beta_j p_j and Ap = Ar - sum beta_j Ap_j into slot ND, <Ap, Ap> and <Ap, r> ------------------------
// (the element-wise expressions — g32_sub_scaled, g32_build_dots, g32_update_one, fold_betas — are gcr32_elem_dev.h's)
template <int ND>
__global__ void __launch_bounds__(RED_THREADS, (ND <= 5 ? 8 : 4))
    g32_build_kernel(const float *__restrict__ r, const float *__restrict__ ar, float *__restrict__ ps, float *__restrict__ aps, int64_t nv, int64_t n,
                     const double *__restrict__ partsB, int nblkB, G32Dev *__restrict__ st, int it, double *__restrict__ partsA, SKIP_ARGS) {
    SKIP_RETURN();
    if (st->stop_a < it || st->stop_u < it) return;
    __shared__ double lds[(2 * ND > 16 ? 16 : 2 * ND > 3 ? 2 * ND : 3) * 17];
    __shared__ float beta[ND ? 2 * ND : 2];
    if constexpr (ND > 0) {
        fold_betas<ND>(partsB, nblkB, st->den, beta, lds);
        __syncthreads();
    }
    double acc[3] = {0., 0., 0.};
    const int64_t npair = n >> 1, half = nv >> 1;
    const float4 *r4 = reinterpret_cast<const float4 *>(r), *ar4 = reinterpret_cast<const float4 *>(ar);
    float4 *ps4 = reinterpret_cast<float4 *>(ps), *aps4 = reinterpret_cast<float4 *>(aps);
    // (a workgroup's base is uniform and the lane's offset 32 bits wide: every stream is addressed from scalar registers plus ONE lane offset)
    for (int64_t b0 = (int64_t)blockIdx.x * RED_THREADS; b0 < npair; b0 += (int64_t)gridDim.x * RED_THREADS) {
        const unsigned t = threadIdx.x;
        if (b0 + t >= npair) break;
        const float4 rr = (r4 + b0)[t];
        float4 p = rr, q = (ar4 + b0)[t];
        // two running pointers walk the slots, two directions' loads in flight
        float4 *pp = ps4 + b0 + t, *qq = aps4 + b0 + t;
#pragma unroll 2
        for (int j = 0; j < ND; j++) {
            const float4 pj = *pp, qj = *qq;
            const float bx = beta[2 * j], by = beta[2 * j + 1];
            pp += half;
            qq += half;
            g32_sub_scaled(bx, by, pj.x, pj.y, p.x, p.y);
            g32_sub_scaled(bx, by, pj.z, pj.w, p.z, p.w);
            g32_sub_scaled(bx, by, qj.x, qj.y, q.x, q.y);
            g32_sub_scaled(bx, by, qj.z, qj.w, q.z, q.w);
        }
        g32_build_dots(q.x, q.y, rr.x, rr.y, acc);
        g32_build_dots(q.z, q.w, rr.z, rr.w, acc);
        *pp = p;      // slot ND
        *qq = q;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
        const int64_t e = n - 1;
        const c32 rr = reinterpret_cast<const c32 *>(r)[e];
        c32 p = rr, q = reinterpret_cast<const c32 *>(ar)[e];
        for (int j = 0; j < ND; j++) {
            const c32 pj = reinterpret_cast<const c32 *>(ps)[(int64_t)j * nv + e], qj = reinterpret_cast<const c32 *>(aps)[(int64_t)j * nv + e];
            g32_sub_scaled(beta[2 * j], beta[2 * j + 1], pj.x, pj.y, p.x, p.y);
            g32_sub_scaled(beta[2 * j], beta[2 * j + 1], qj.x, qj.y, q.x, q.y);
        }
        g32_build_dots(q.x, q.y, rr.x, rr.y, acc);
        reinterpret_cast<c32 *>(ps)[(int64_t)ND * nv + e] = p;
        reinterpret_cast<c32 *>(aps)[(int64_t)ND * nv + e] = q;
    }
    block_sums_to_slab<3>(acc, lds, partsA, blockIdx.x);
}

// ---- update: alpha, x += alpha p, r -= alpha Ap, |r|^2, the step counter -------------------------------------------------------------
__global__ void __launch_bounds__(RED_THREADS, 8)
    g32_update_kernel(float *__restrict__ x, float *__restrict__ r, const float *__restrict__ p, const float *__restrict__ ap, int64_t n,
                      const double *__restrict__ partsA, int nblkA, G32Dev *__restrict__ st, int it, int slot, double *__restrict__ S2, SKIP_ARGS) {
    SKIP_RETURN();
    if (st->stop_a < it) return;
    __shared__ double lds[3 * 17];
    double v[3];
    fold_partials<3>(partsA, nblkA, RED_MAX_BLOCKS, v, lds);
    if (!(v[0] > 0.)) {   // <Ap, Ap> exactly zero: the solve is over with what x holds
        if (blockIdx.x == 0 && threadIdx.x == 0) st->stop_u = it - 1;
        return;
    }
    const float ax = uniform((float)(v[1] / v[0])), ay = uniform((float)(v[2] / v[0]));   // formed in fp64, rounded once
    double acc[1] = {0.};
    const int64_t npair = n >> 1;
    float4 *x4 = reinterpret_cast<float4 *>(x), *r4 = reinterpret_cast<float4 *>(r);
    const float4 *p4 = reinterpret_cast<const float4 *>(p), *q4 = reinterpret_cast<const float4 *>(ap);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
        float4 xv = x4[i], rv = r4[i];
        const float4 pv = p4[i], qv = q4[i];
        g32_update_one(ax, ay, pv.x, pv.y, qv.x, qv.y, xv.x, xv.y, rv.x, rv.y, acc[0]);
        g32_update_one(ax, ay, pv.z, pv.w, qv.z, qv.w, xv.z, xv.w, rv.z, rv.w, acc[0]);
        x4[i] = xv;
        r4[i] = rv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
        const int64_t e = n - 1;
        c32 xv = reinterpret_cast<c32 *>(x)[e], rv = reinterpret_cast<c32 *>(r)[e];
        const c32 pv = reinterpret_cast<const c32 *>(p)[e], qv = reinterpret_cast<const c32 *>(ap)[e];
        g32_update_one(ax, ay, pv.x, pv.y, qv.x, qv.y, xv.x, xv.y, rv.x, rv.y, acc[0]);
        reinterpret_cast<c32 *>(x)[e] = xv;
        reinterpret_cast<c32 *>(r)[e] = rv;
    }
    const double mine = block_sum_owner<1>(acc, lds);
    if (threadIdx.x == 0) S2[RED_MAX_BLOCKS + blockIdx.x] = mine;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->n_iter = it; st->den[slot] = v[0]; }
}

// ---- exit: y = fp64(x); st != NULL: |r| / |f| behind the last step ------------------------------------------------------------------
__global__ void __launch_bounds__(RED_THREADS) g32_exit_kernel(const float *__restrict__ x, cplx *__restrict__ y, int64_t n, const double *__restrict__ S2,
                                                               int nblkS, G32Dev *__restrict__ st, SKIP_ARGS) {
    SKIP_RETURN();
    __shared__ double lds[2 * 17];
    const int64_t npair = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4 *>(x)[i];
        y[2 * i] = make_double2((double)v.x, (double)v.y);
        y[2 * i + 1] = make_double2((double)v.z, (double)v.w);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const c32 v = reinterpret_cast<const c32 *>(x)[n - 1];
        y[n - 1] = make_double2((double)v.x, (double)v.y);
    }
    if (st && blockIdx.x == 0) {
        double s2[2];
        fold_partials<2>(S2, nblkS, RED_MAX_BLOCKS, s2, lds);
        if (threadIdx.x == 0) st->rel = s2[0] > 0. ? sqrt(s2[1] / s2[0]) : 0.;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
void gcr32_destroy(Gcr32State *g) {
    if (!g) return;
    hipFree(g->val); hipFree(g->tail_val); hipFree(g->col); hipFree(g->tile_tail); hipFree(g->tail_rows); hipFree(g->tail_ptr); hipFree(g->tail_col);
    hipFree(g->r); hipFree(g->ar); hipFree(g->x); hipFree(g->ps); hipFree(g->aps);
    hipFree(g->S2); hipFree(g->partsA); hipFree(g->partsB); hipFree(g->st);
    gcr32_eo_destroy(g->eo);
    gcr32_multi_destroy(g->mw);
    delete g;
}
int64_t gcr32_nnz(const Gcr32State *g) { return g->nnz; }

static int g32_alloc_slots(Gcr32State *g, int restart) {
    float *ps = nullptr, *aps = nullptr;
    MGCR_TRY(g32_alloc(&ps, (size_t)2 * g->nv * restart));
    int rc = g32_alloc(&aps, (size_t)2 * g->nv * restart);
    if (rc != MGCR_OK) { hipFree(ps); return rc; }
    hipFree(g->ps); hipFree(g->aps);
    g->ps = ps; g->aps = aps;
    return MGCR_OK;
}

// the inner parameters: what the operator refuses (nothing is changed then)
int g32_check_param(const mgcr_gcr_param *p, const char *who) {
    MGCR_CHECK(p->truncation >= 0 && p->restart >= 0, MGCR_ERR_INVALID, "%s: negative GCR parameter", who);
    std::string err;
    if (!gcr32_param_ok(p->truncation, p->restart, p->max_iter, p->left_precond || p->right_precond, p->use_x0 != 0, p->flexible != 0,
                        p->profile_spmv != 0, &err)) {
        set_error("%s: %s", who, err.c_str());
        return MGCR_ERR_UNSUPPORTED;
    }
    MGCR_CHECK(p->max_iter >= 1, MGCR_ERR_INVALID, "%s: max_iter = %d, the inner solve enqueues at least one step", who, (int)p->max_iter);
    MGCR_CHECK(p->tol >= 0. && std::isfinite(p->tol), MGCR_ERR_INVALID, "%s: tol must be finite and not negative", who);
    return MGCR_OK;
}

int g32_check_k(const double k_ri[2], c32 *k32, const char *who) {
    MGCR_CHECK(k_ri[0] != 0. || k_ri[1] != 0., MGCR_ERR_INVALID, "%s: No k value supplied for Dirac Operator!", who);
    float re, im;
    MGCR_CHECK(gcr32_to_float(k_ri[0], &re) && gcr32_to_float(k_ri[1], &im), MGCR_ERR_INVALID, "%s: k is not finite in single precision", who);
    *k32 = make_float2(re, im);
    return MGCR_OK;
}

static G32Mat g32_mat(const Gcr32State *g) {
    return G32Mat{g->val, g->col, g->npad, g->W, g->tile_tail, g->tail_rows, g->tail_ptr, g->tail_col, g->tail_val};
}

// "the apply of this operator": Ar = A32 r and the partials of <Ap_j, Ar> — one launch for the square form, two for the even-odd one
static int g32_launch_apply(Gcr32State *g, int nd, int it, SkipRef sk) {
    if (g->eo) return gcr32_eo_launch_apply(g, nd, it, sk);
    const int ga = red_grid(g->n), gs = red_grid(g->n >> 1);
    const double tol2 = g->tol * g->tol;
    return dispatch_bool(g->real, [&](auto real) {
        return dispatch_nd<0, GCR32_MAX_RESTART - 1>(nd, [&](auto ndc) {
            return launch(g32_apply_kernel<decltype(ndc)::value, decltype(real)::value>, ga, RED_THREADS, 0, g32_mat(g), (const c32 *)g->r, (c32 *)g->ar,
                          (const c32 *)g->aps, g->nv, g->n, g->dirac ? 1 : 0, g->k32, (const double *)g->S2, gs, tol2, g->st, it, g->partsB, sk.p, sk.it);
        });
    });
}

int gcr32_apply(Op *op, const cplx *f, cplx *y, int64_t n, Gcr32Gate gate) {
    Gcr32State *g = op->g32;
    MGCR_CHECK(g->n == n, MGCR_ERR_INVALID, "low-precision GCR of %lld rows applied to a Field of %lld entries", (long long)g->n, (long long)n);
    const SkipRef sk = get_apply_skip();
    const int ga = red_grid(n), gs = red_grid(n >> 1);
    MGCR_TRY(launch(g32_entry_kernel, gs, RED_THREADS, 0, f, g->r, g->x, n, g->st, g->S2, gate, g_dev_counts, g->max_iter, sk.p, sk.it));
    for (int it = 1; it <= g->max_iter; it++) {
        const int nd = (it - 1) % g->restart;   // directions stored when the step starts; the new one goes into slot nd
        MGCR_TRY(g32_launch_apply(g, nd, it, sk));
        const int brc = dispatch_nd<0, GCR32_MAX_RESTART - 1>(nd, [&](auto ndc) {
            return launch(g32_build_kernel<decltype(ndc)::value>, gs, RED_THREADS, 0, (const float *)g->r, (const float *)g->ar, g->ps, g->aps, g->nv, n,
                          (const double *)g->partsB, ga, g->st, it, g->partsA, sk.p, sk.it);
        });
        MGCR_TRY(brc);
        MGCR_TRY(launch(g32_update_kernel, gs, RED_THREADS, 0, g->x, g->r, (const float *)(g->ps + (size_t)2 * g->nv * nd),
                        (const float *)(g->aps + (size_t)2 * g->nv * nd), n, (const double *)g->partsA, gs, g->st, it, nd, g->S2, sk.p, sk.it));
    }
    MGCR_TRY(launch(g32_exit_kernel, gs, RED_THREADS, 0, (const float *)g->x, y, n, (const double *)g->S2, gs, g->st, sk.p, sk.it));
    return MGCR_OK;
}

// The slots of an fp64 solve that take the operator (gcr.hip): right_precond with flexible = 1 only — the inner solve stops on a
// tolerance, so it is not a linear map
int gcr32_slot_check(const mgcr_gcr_param *p, const Op *A) {
    const Op *l = (const Op *)p->left_precond, *r = (const Op *)p->right_precond;
    MGCR_CHECK(!l || l->kind != OP_GCR32, MGCR_ERR_UNSUPPORTED,
               "a low-precision GCR stops on a tolerance and is not a linear map: it goes into the right_precond slot with flexible = 1, not into left_precond");
    if (!r || r->kind != OP_GCR32) return MGCR_OK;
    MGCR_CHECK(p->flexible, MGCR_ERR_UNSUPPORTED,
               "a low-precision GCR stops on a tolerance and is not a linear map: set flexible = 1 to use it as the right preconditioner");
    if (A) {
        const Op *b0 = op_matrix(A);
        MGCR_CHECK(!A->dist && !A->comm && !(b0 && (b0->dist || b0->comm)), MGCR_ERR_UNSUPPORTED,
                   "a low-precision GCR cannot precondition a distributed operator");
        MGCR_CHECK(A->dim == r->dim, MGCR_ERR_INVALID, "the low-precision GCR has %lld rows, the operator of the solve %lld", (long long)r->dim,
                   (long long)A->dim);
        if (r->g32->eo) MGCR_TRY(gcr32_eo_slot_check(r->g32->eo, A));
    }
    return MGCR_OK;
}

// r, Ar, x, the restart slots, the partial slabs, the state words and — with the first operator — the library's two counters
int g32_alloc_iteration(Gcr32State *g) {
    int rc = MGCR_OK;
    if (rc == MGCR_OK) rc = g32_alloc(&g->r, (size_t)2 * g->nv);
    if (rc == MGCR_OK) rc = g32_alloc(&g->ar, (size_t)2 * g->nv);
    if (rc == MGCR_OK) rc = g32_alloc(&g->x, (size_t)2 * g->nv);
    if (rc == MGCR_OK) rc = g32_alloc_slots(g, g->restart);
    if (rc == MGCR_OK) rc = g32_alloc(&g->S2, (size_t)2 * RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = g32_alloc(&g->partsA, (size_t)3 * RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = g32_alloc(&g->partsB, (size_t)2 * GCR32_MAX_RESTART * RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = g32_alloc(&g->st, 1);
    if (rc == MGCR_OK && hipMemset(g->st, 0, sizeof(G32Dev)) != hipSuccess) rc = MGCR_ERR_HIP;
    if (rc == MGCR_OK && !g_dev_counts) {   // the library's two device-side counters: made with the first operator, zeroed on the library's stream
        rc = g32_alloc(&g_dev_counts, 2);
        if (rc == MGCR_OK && hipMemsetAsync(g_dev_counts, 0, 2 * sizeof(long long), ctx().stream) != hipSuccess) rc = MGCR_ERR_HIP;
    }
    if (rc == MGCR_OK && hipDeviceSynchronize() != hipSuccess) rc = MGCR_ERR_HIP;   // (the memset above went to the null stream)
    return rc;
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)
#define G32_CHECK(op, who) MGCR_CHECK((op) && (op)->kind == OP_GCR32 && (op)->g32, MGCR_ERR_INVALID, "%s: not a low-precision GCR", who)

extern "C" {

int mgcr_gcr32_create(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const double *k_ri, const mgcr_gcr_param *inner,
                      mgcr_op_t *out) {
    const char *who = "mgcr_gcr32_create";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && inner && n >= 0 && (col || rowptr[n] == 0) && (val_ri || rowptr[n] == 0), MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_TRY(g32_check_param(inner, who));
    c32 k32 = make_float2(0.f, 0.f);
    if (k_ri) MGCR_TRY(g32_check_k(k_ri, &k32, who));
    Gcr32Plan plan;
    std::string err;
    if (!gcr32_plan_build(n, rowptr, col, val_ri, G32_TILE, &plan, &err)) {
        set_error("%s: %s", who, err.c_str());
        return MGCR_ERR_INVALID;
    }
    LOCK();
    Gcr32State *g = new Gcr32State();
    g->n = n; g->nv = (n + 3) / 4 * 4; g->nnz = plan.nnz; g->n_tail_rows = (int64_t)plan.tail_rows.size(); g->stored_bytes = plan.stored_bytes();
    g->W = plan.W; g->npad = plan.npad; g->real = plan.real_slab; g->dirac = k_ri != nullptr;
    if (k_ri) { g->k_ri[0] = k_ri[0]; g->k_ri[1] = k_ri[1]; g->k32 = k32; }
    g->restart = inner->restart; g->max_iter = inner->max_iter; g->tol = inner->tol;
    int rc = g32_upload(&g->val, plan.ell_val);
    if (rc == MGCR_OK) rc = g32_upload(&g->col, plan.ell_col);
    if (rc == MGCR_OK) rc = g32_upload(&g->tile_tail, plan.tile_tail);
    if (rc == MGCR_OK) rc = g32_upload(&g->tail_rows, plan.tail_rows);
    if (rc == MGCR_OK) rc = g32_upload(&g->tail_ptr, plan.tail_ptr);
    if (rc == MGCR_OK) rc = g32_upload(&g->tail_col, plan.tail_col);
    if (rc == MGCR_OK) rc = g32_upload(&g->tail_val, plan.tail_val);
    if (rc == MGCR_OK) rc = g32_alloc_iteration(g);
    if (rc != MGCR_OK) { gcr32_destroy(g); return rc; }
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_GCR32;
    op->dim = op->nrow = n;
    op->g32 = g;
    *out = op;
    return MGCR_OK;
}

// The value travels in the kernel arguments of every launch: what is already enqueued keeps the old one.
int mgcr_gcr32_set_k(mgcr_op_t op, const double k_ri[2]) {
    const char *who = "mgcr_gcr32_set_k";
    G32_CHECK(op, who);
    MGCR_CHECK(k_ri, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_CHECK(op->g32->dirac, MGCR_ERR_INVALID, "%s: the operator was made in matrix form and has no k", who);
    c32 k32;
    MGCR_TRY(g32_check_k(k_ri, &k32, who));
    LOCK();
    if (op->g32->eo) MGCR_TRY(gcr32_eo_set_k(op->g32, k_ri, who));   // a and 1 / a_o follow k; refused: nothing changes
    op->g32->k_ri[0] = k_ri[0]; op->g32->k_ri[1] = k_ri[1];
    op->g32->k32 = k32;
    return MGCR_OK;
}

int mgcr_gcr32_set_param(mgcr_op_t op, const mgcr_gcr_param *inner) {
    const char *who = "mgcr_gcr32_set_param";
    G32_CHECK(op, who);
    MGCR_CHECK(inner, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_TRY(g32_check_param(inner, who));
    LOCK();
    Gcr32State *g = op->g32;
    if (inner->restart != g->restart) {
        MGCR_HIP(hipStreamSynchronize(ctx().stream));   // nothing queued may still use the old slots
        MGCR_TRY(g32_alloc_slots(g, inner->restart));
    }
    g->restart = inner->restart; g->max_iter = inner->max_iter; g->tol = inner->tol;
    return MGCR_OK;
}

int mgcr_gcr32_info(mgcr_op_t op, int64_t *n, int32_t *ell_width, int64_t *tail_rows, int32_t *real_slab, int64_t *stored_bytes) {
    G32_CHECK(op, "mgcr_gcr32_info");
    const Gcr32State *g = op->g32;
    MGCR_CHECK(!g->eo, MGCR_ERR_UNSUPPORTED, "mgcr_gcr32_info: the operator is in even-odd form and has two slabs: ask mgcr_gcr32_eo_info");
    if (n) *n = g->n;
    if (ell_width) *ell_width = g->W;
    if (tail_rows) *tail_rows = g->n_tail_rows;
    if (real_slab) *real_slab = g->real ? 1 : 0;
    if (stored_bytes) *stored_bytes = g->stored_bytes;
    return MGCR_OK;
}

int mgcr_gcr32_apply_matrix(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y) {
    const char *who = "mgcr_gcr32_apply_matrix";
    MGCR_TRY(require_ctx());
    G32_CHECK(op, who);
    MGCR_CHECK(x && y, MGCR_ERR_INVALID, "%s: null argument", who);
    Gcr32State *g = op->g32;
    MGCR_CHECK(x->n == g->n && y->n == g->n, MGCR_ERR_INVALID, "%s: the operator has %lld rows, the Fields %lld and %lld entries", who, (long long)g->n,
               (long long)x->n, (long long)y->n);
    LOCK();
    const int gs = red_grid(g->n >> 1);
    const SkipRef none{};
    MGCR_TRY(launch(g32_entry_kernel, gs, RED_THREADS, 0, (const cplx *)x->d, g->r, g->x, g->n, (G32Dev *)nullptr, g->S2, Gcr32Gate(), (long long *)nullptr, 0, none.p, none.it));
    MGCR_TRY(g32_launch_apply(g, 0, 0, none));
    return launch(g32_exit_kernel, gs, RED_THREADS, 0, (const float *)g->ar, y->w(), g->n, (const double *)g->S2, gs, (G32Dev *)nullptr, none.p, none.it);
}

int mgcr_gcr32_last(mgcr_op_t op, int32_t *n_iter, double *rel_res) {
    MGCR_TRY(require_ctx());
    G32_CHECK(op, "mgcr_gcr32_last");
    LOCK();
    Context &c = ctx();
    static_assert(sizeof(G32Dev) <= 64 * sizeof(double), "the mailbox holds the state");
    MGCR_HIP(hipMemcpyAsync(c.h_mail, op->g32->st, sizeof(G32Dev), hipMemcpyDeviceToHost, c.stream));
    MGCR_HIP(hipStreamSynchronize(c.stream));
    const G32Dev *h = (const G32Dev *)c.h_mail;
    if (n_iter) *n_iter = h->n_iter;
    if (rel_res) *rel_res = h->rel;
    return MGCR_OK;
}

}  // extern "C"
