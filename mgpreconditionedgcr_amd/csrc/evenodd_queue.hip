// The queued even-odd scan (mgcr_eo_solve_queue): see the driver's comment below.  Its kernels move MASKED columns between the systems'
// full Fields and the half blocks of a batched Schur solve; everything else is gcr_queue_run (gcr_multi.hip) and the k-wide
// shifted half applies of evenodd_multi.hip.
#include <algorithm>

#include "evenodd_multi.h"
#include "gcr_dev.h"      // LND: the longest restart cycle of the batched solves
#include "queue_plan.h"   // host only: the slots of a cycle as the queued solve counts them

namespace mgcr {

// ------------------------------------------------------------------------------------------------
// The queued even-odd scan (mgcr_eo_solve_queue): nsys systems (1 - k_s D) x_s = b_s on full Fields stream through the W = min(width,
// nsys) columns of ONE batched Schur solve on n_e rows.  Schedule and steps are gcr_queue_run's (gcr_multi.hip; queue_plan.h
// unchanged), with a MultiEvenOddDiracOp of W columns as the slot operator: its k_j and k_j^2 travel in the kernel arguments of
// every apply, and admitting system s into slot j sets entry j.  What the queue cannot do on its own — the systems are full Fields,
// its columns even halves — happens in the hooks below.  Every launch is enqueued by the host in stream order.
//   admission point (mask = the admitted slots), whatever the number of columns admitted:
//     eoq_gather_kernel      b_e -> W_BE, b_o -> W_BO, x_e -> the x block: the admitted columns only, through even[] / odd[]
//     eom_shift_apply(D_eo)  W_BHAT = W_BE - (-k_j) D_eo W_BO, all W columns (one k-wide launch; two, the second eom_sub_scaled_kernel,
//                            for a half with a CSR tail) — a column not admitted is computed on what its slot holds; nothing of it
//                            is stored
//     eoq_copy_kernel        the admitted columns of W_BHAT -> the b block and, without x0, r and P0
//     then the queue's own admission: with x0 the Schur apply of the x block and q_r0_kernel; the Schur apply of r,
//     m_init_partials_kernel<KC, true>, q_admit_state_kernel.  In all 4 (5 with x0) passes and 1 shifted D_eo + 1 (2) Schur applies.
//   retirement point (mask = the slots found stopped):
//     m_pending_x_kernel<KC, XBlock>  the pending x updates of the retiring columns -> W_XE (gcr_multi.hip: its work-block sink)
//     eom_shift_apply(D_oe)  W_XO = W_BO - (-k_j) D_oe W_XE, all W columns (one launch, two with a tail)
//     eoq_scatter_kernel     the retiring columns of W_XE and W_XO -> the systems' full Fields, through even[] / odd[]
// W_BO is the block of the b_o in flight: column j is written when slot j is admitted and read when it retires.
// Storage: the queue's own (MWork at n_e rows, W columns) plus the slot operator with its work blocks (W_BE, W_BO, W_BHAT, W_XE,
// W_XO, t; W_UE / W_UO for halves with a tail), kept in g_eoq from call to call, re-made when n_e, n_o or W change and released by
// multi_release (mgcr_finalize).
// ------------------------------------------------------------------------------------------------
struct EoqFields {   // per slot: the system's full Fields (by value in the kernel arguments)
    const cplx *b[MV_MAX_K];
    cplx *x[MV_MAX_K];
};

// Masked columns of full Fields <-> columns of half blocks; the lanes and rows of eom_split_kernel (KP lanes per row, one 128-bit
// access each on the block side; lane c serves column c, whose Fields it looks up once)
template <int KP>
__global__ void __launch_bounds__(RED_THREADS) eoq_gather_kernel(unsigned mask, EoqFields f, cplx *__restrict__ be, cplx *__restrict__ bo,
                                                                 cplx *__restrict__ xe, const int32_t *__restrict__ ev,
                                                                 const int32_t *__restrict__ od, int64_t ne, int64_t no, int k) {
    constexpr int ROWS = RED_THREADS / KP;
    const int c = (int)threadIdx.x & (KP - 1);
    if (c >= k || !((mask >> c) & 1u)) return;
    const cplx *__restrict__ bs = f.b[c];
    const cplx *__restrict__ xs = f.x[c];
    for (int64_t i = (int64_t)blockIdx.x * ROWS + (int)threadIdx.x / KP; i < ne + no; i += (int64_t)gridDim.x * ROWS) {
        if (i < ne) {
            const int64_t s = ev[i];
            be[i * k + c] = bs[s];
            xe[i * k + c] = xs[s];
        } else {
            bo[(i - ne) * k + c] = bs[od[i - ne]];
        }
    }
}
template <int KP>
__global__ void __launch_bounds__(RED_THREADS) eoq_scatter_kernel(unsigned mask, EoqFields f, const cplx *__restrict__ xe, const cplx *__restrict__ xo,
                                                                  const int32_t *__restrict__ ev, const int32_t *__restrict__ od, int64_t ne,
                                                                  int64_t no, int k) {
    constexpr int ROWS = RED_THREADS / KP;
    const int c = (int)threadIdx.x & (KP - 1);
    if (c >= k || !((mask >> c) & 1u)) return;
    cplx *__restrict__ xs = f.x[c];
    for (int64_t i = (int64_t)blockIdx.x * ROWS + (int)threadIdx.x / KP; i < ne + no; i += (int64_t)gridDim.x * ROWS) {
        if (i < ne) xs[ev[i]] = xe[i * k + c];
        else xs[od[i - ne]] = xo[(i - ne) * k + c];
    }
}
// the masked columns of src -> those of d0 and, where given, d1 and d2 (blocks of n rows)
template <int KP>
__global__ void __launch_bounds__(RED_THREADS) eoq_copy_kernel(unsigned mask, const cplx *__restrict__ src, cplx *__restrict__ d0, cplx *__restrict__ d1,
                                                               cplx *__restrict__ d2, int64_t n, int k) {
    constexpr int ROWS = RED_THREADS / KP;
    const int c = (int)threadIdx.x & (KP - 1);
    if (c >= k || !((mask >> c) & 1u)) return;
    for (int64_t i = (int64_t)blockIdx.x * ROWS + (int)threadIdx.x / KP; i < n; i += (int64_t)gridDim.x * ROWS) {
        const cplx v = src[i * k + c];
        d0[i * k + c] = v;
        if (d1) d1[i * k + c] = v;
        if (d2) d2[i * k + c] = v;
    }
}
// launches kernel<KP> over `rows` rows of k columns
#define EOQ_LAUNCH_KP(kernel, rows, k, ...)                                                                                      \
    do {                                                                                                                         \
        const int kp__ = (k) <= 1 ? 1 : (k) <= 2 ? 2 : (k) <= 4 ? 4 : (k) <= 8 ? 8 : 16;                                         \
        const unsigned grid__ = (unsigned)red_grid((rows) * kp__);                                                               \
        if (kp__ == 1) return launch(kernel<1>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 2) return launch(kernel<2>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 4) return launch(kernel<4>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        if (kp__ == 8) return launch(kernel<8>, grid__, RED_THREADS, 0, __VA_ARGS__);                                            \
        return launch(kernel<16>, grid__, RED_THREADS, 0, __VA_ARGS__);                                                          \
    } while (0)
static int eoq_gather(const EoState *e, unsigned mask, const EoqFields &f, cplx *be, cplx *bo, cplx *xe, int k) {
    EOQ_LAUNCH_KP(eoq_gather_kernel, e->n, k, mask, f, be, bo, xe, (const int32_t *)e->d_even, (const int32_t *)e->d_odd, e->ne, e->no, k);
}
static int eoq_scatter(const EoState *e, unsigned mask, const EoqFields &f, const cplx *xe, const cplx *xo, int k) {
    EOQ_LAUNCH_KP(eoq_scatter_kernel, e->n, k, mask, f, xe, xo, (const int32_t *)e->d_even, (const int32_t *)e->d_odd, e->ne, e->no, k);
}
static int eoq_copy(unsigned mask, const cplx *src, cplx *d0, cplx *d1, cplx *d2, int64_t n, int k) {
    EOQ_LAUNCH_KP(eoq_copy_kernel, n, k, mask, src, d0, d1, d2, n, k);
}
#undef EOQ_LAUNCH_KP

namespace {
// the slot operator, kept from call to call with its work blocks
struct EoQueueWork {
    mgcr_op_s *slot = nullptr;
    int64_t ne = -1, no = -1;
    void release() {
        if (!slot) return;
        if (ctx().ready) hipStreamSynchronize(ctx().stream);
        eo_multi_destroy(slot->eom);
        delete slot;
        slot = nullptr;
    }
    // a MultiEvenOddDiracOp of k columns on eo's halves; every slot starts with k_j = 1 (an empty slot's column is never stored)
    Op *prepare(Op *eo, int k) {
        const EoState *e = eo->eo;
        if (slot && (ne != e->ne || no != e->no || slot->nk != k)) release();
        if (!slot) {
            slot = new mgcr_op_s();
            slot->kind = OP_DIRAC_EO_MULTI;
            slot->eom = new EoMultiState();
            ne = e->ne; no = e->no;
        }
        slot->dim = slot->nrow = e->ne;
        slot->nk = k;
        slot->eom->eo = eo;
        for (int j = 0; j < MV_MAX_K; j++) slot->ks[j] = slot->eom->ks2.v[j] = make_double2(j < k ? 1. : 0., 0.);
        return slot;
    }
};
EoQueueWork g_eoq;

struct EoQueueHooks : QueueHooks {
    Op *slot = nullptr;
    const EoState *e = nullptr;
    const cplx *const *rhs = nullptr;
    cplx *const *x = nullptr;
    const cplx *ks = nullptr;
    EoqFields f{};
    cplx *be = nullptr, *bo = nullptr, *bhat = nullptr, *xe = nullptr, *xo = nullptr;

    int init() {
        MGCR_TRY(eom_work(slot, EoState::W_BE, &be));
        MGCR_TRY(eom_work(slot, EoState::W_BO, &bo));
        MGCR_TRY(eom_work(slot, EoState::W_BHAT, &bhat));
        MGCR_TRY(eom_work(slot, EoState::W_XE, &xe));
        return eom_work(slot, EoState::W_XO, &xo);
    }
    int admit(unsigned mask, int m, const int *slots, const int *systems, cplx *xb, cplx *bb, cplx *r, cplx *p0, bool use_x0) override {
        const int k = slot->nk;
        for (int i = 0; i < m; i++) {
            const int j = slots[i], s = systems[i];
            f.b[j] = rhs[s];
            f.x[j] = x[s];
            slot->ks[j] = ks[s];
            slot->eom->ks2.v[j] = host_cmul(ks[s], ks[s]);
        }
        MGCR_TRY(eoq_gather(e, mask, f, be, bo, xb, k));
        MGCR_TRY(eom_shift_apply(slot, 0, bo, bhat, eom_negated(slot), be));
        return eoq_copy(mask, bhat, bb, use_x0 ? nullptr : r, use_x0 ? nullptr : p0, e->ne, k);
    }
    cplx *retire_block() override { return xe; }
    int retire(unsigned mask) override {
        MGCR_TRY(eom_shift_apply(slot, 1, xe, xo, eom_negated(slot), bo));
        return eoq_scatter(e, mask, f, xe, xo, slot->nk);
    }
};
}  // namespace

void eo_queue_release() { g_eoq.release(); }

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_eo_solve_queue(mgcr_op_t eo, const mgcr_gcr_param *param, int32_t width, int32_t nsys, const mgcr_vec_t *rhs_full, const mgcr_vec_t *x_full,
                        const double *k_ri, double *hist, int32_t hist_cap, int32_t *n_iter, int32_t *converged) {
    const char *who = "mgcr_eo_solve_queue";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(eo && param && rhs_full && x_full && k_ri, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_REFUSE_GCR32(eo, who);
    MGCR_CHECK(eo->kind == OP_DIRAC_EO && eo->eo, MGCR_ERR_INVALID,
               "%s: the operator must be an even-odd preconditioned DiracOp (its halves carry the queue; the hopping parameters come per system)", who);
    MGCR_CHECK(!eo->eo->has_diag, MGCR_ERR_UNSUPPORTED,
               "%s: the operator carries a site diagonal (mgcr_eo_create_diag): 1 - k_s d would differ from column to column, which the scans "
               "do not support; solve one k at a time with mgcr_eo_solve", who);
    MGCR_CHECK(!eo->eo->has_block, MGCR_ERR_UNSUPPORTED,
               "%s: the operator carries a dense block per site (mgcr_eo_create_block): dense site blocks would be per column, which the scans "
               "do not support; solve one k at a time with mgcr_eo_solve", who);
    MGCR_CHECK(width >= 1 && width <= MV_MAX_K, MGCR_ERR_INVALID, "%s: width = %d slots, 1 .. %d are supported", who, (int)width, MV_MAX_K);
    MGCR_CHECK(nsys >= 1, MGCR_ERR_INVALID, "%s: nsys = %d systems", who, (int)nsys);
    // (the restrictions of mgcr_eo_multi_solve, checked before anything is enqueued)
    MGCR_CHECK(param->truncation >= 0 && param->restart >= 0 && param->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_CHECK(param->truncation == 0, MGCR_ERR_UNSUPPORTED, "%s: truncation mode is not supported (restart mode only)", who);
    MGCR_CHECK(param->restart != 0, MGCR_ERR_UNSUPPORTED, "%s: restart mode only (restart != 0)", who);
    MGCR_CHECK(!param->left_precond && !param->right_precond, MGCR_ERR_UNSUPPORTED, "%s: preconditioners are not supported", who);
    MGCR_CHECK(!param->flexible && !param->profile_spmv, MGCR_ERR_UNSUPPORTED, "%s: flexible / profile_spmv are not supported", who);
    const int k = width < nsys ? width : nsys;
    MGCR_CHECK(QueuePlan(k, nsys, param->restart, param->max_iter, param->check_every).storage <= LND, MGCR_ERR_UNSUPPORTED,
               "batched GCR: restart cycles of at most %d steps (the lean cycle) are supported", LND);
    const EoState *e = eo->eo;
    std::vector<const void *> xs, bs;
    std::vector<cplx> ks((size_t)nsys);
    for (int32_t s = 0; s < nsys; s++) {
        MGCR_CHECK(rhs_full[s] && x_full[s], MGCR_ERR_INVALID, "%s: system %d has a null Field", who, (int)s);
        for (const mgcr_vec_t v : {rhs_full[s], x_full[s]})
            MGCR_CHECK(v->n == e->n, MGCR_ERR_INVALID,
                       "%s: a Field of system %d has %lld entries, the %lld of the full system are needed%s", who, (int)s, (long long)v->n,
                       (long long)e->n, v->n == e->ne ? " (it has the length of the even half: the queue takes full Fields)" : "");
        xs.push_back(x_full[s]->d);
        bs.push_back(rhs_full[s]->d);
        MGCR_CHECK(k_ri[2 * s] != 0. || k_ri[2 * s + 1] != 0., MGCR_ERR_INVALID, "%s: k[%d] is zero (No k value supplied for Dirac Operator!)", who, (int)s);
        ks[(size_t)s] = make_double2(k_ri[2 * s], k_ri[2 * s + 1]);
    }
    if (e->n > 0) {   // the x Fields are written while other systems still read their right-hand sides
        std::sort(xs.begin(), xs.end());
        std::sort(bs.begin(), bs.end());
        MGCR_CHECK(std::adjacent_find(xs.begin(), xs.end()) == xs.end(), MGCR_ERR_INVALID, "%s: the x Fields must be pairwise distinct", who);
        for (const void *q : xs)
            MGCR_CHECK(!std::binary_search(bs.begin(), bs.end(), q), MGCR_ERR_INVALID, "%s: an x Field is also a right-hand side", who);
    }
    LOCK();
    std::vector<const cplx *> bp((size_t)nsys);
    std::vector<cplx *> xp((size_t)nsys);
    for (int32_t s = 0; s < nsys; s++) {
        bp[(size_t)s] = rhs_full[s]->d;
        xp[(size_t)s] = x_full[s]->w();
    }
    EoQueueHooks hk;
    hk.slot = g_eoq.prepare(eo, k);
    hk.e = e;
    hk.rhs = bp.data();
    hk.x = xp.data();
    hk.ks = ks.data();
    MGCR_TRY(hk.init());
    return gcr_queue_run(hk.slot, *param, k, nsys, nullptr, nullptr, nullptr, e->ne, hist, hist_cap, n_iter, converged, &hk);
}

}  // extern "C"
