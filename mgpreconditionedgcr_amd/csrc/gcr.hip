// Device-resident GCR (restarted / truncated / full) — the reference's GCR<T>::solve
// (src/GCR.h:158-302) re-designed for MI355X:
//
//   * x, r and the stored directions live in HBM for the whole solve; p and Ap are not separate
//     vectors but the ring slot that was written last (the reference copies them, :286-287);
//   * per iteration three kernels instead of ~90 vector passes; which of their forms a solve launches is
//     decided once, in gcr_plan (SolvePlan), and enqueued by gcr_start and gcr_step's phases:
//        xr_update   x += a p, r -= a Ap, |r|^2 partials                         6 V  (3 V when the
//                    x update is deferred to the end of the restart cycle, see xr_update_kernel)
//        apply+dots  Ar = A r and the <Ar, Aps[i]> partials for all stored i      B_matrix + (2+lim) V
//                    (gcr_fused.hip: one kernel for a Sparse / DiracOp stored one thread per row; else
//                    the operator's own apply followed by multidot_kernel, (1+lim) V more)
//        build       p' = r - sum b_i ps[i], Ap' = Ar - sum b_i Aps[i] written straight into the
//                    ring slot, plus <r,Ap'> and <Ap',Ap'> partials and the step's bookkeeping
//                    (history entry, convergence predicate)                        (4+2 lim) V
//     = B_matrix + (9 + 3 lim) V of HBM traffic per iteration in the classic form, and
//   * LEAN (SolvePlan::lean): inside a restart cycle the directions p_k are never formed.  Only x needs them, and x is
//     updated once per cycle, so the solver keeps what p_k is a combination of — the cycle's first direction P0 and the
//     residuals (or M r, flexible mode) D_1..D_k the later directions were started from — plus the small triangular table of
//     coefficients p_k = t_k P0 + sum_m T_km D_m on the device.  The residual ring costs nothing (xr_update writes r into the
//     slot instead of in place), build shrinks from (4+2 lim) V to (3+lim) V, and the step that closes the cycle applies
//     x += sum_k alpha_k p_k and forms the next P0 from the same streams the classic closing step reads.  r, Ap and every
//     scalar follow the same recurrences with the same bits; x differs by rounding only;
//   * all scalars (alpha, beta_i, norms, the iteration counter, the convergence flag and the
//     residual history) stay on the device.  Reductions are two-stage and deterministic: producers
//     write per-workgroup partials, consumers fold them in a fixed order (reduce.h), so the
//     history is reproducible run to run.  The host only looks at the device-side stop predicate
//     every `check_every` iterations; once it is set every later kernel returns immediately, so x, r
//     and the history are exactly those of the converged step;
//   * the work vectors belong to the solver object and are re-used from solve to solve;
//   * streams touched once per iteration (old direction slots; the matrix in spmv.hip) are accessed
//     non-temporally so that r, Ar and the newest Ap survive in L2 / Infinity Cache between kernels;
//   * used as an Operator (smoother / coarse solver / preconditioner, src/GCR.h:62-68) a solve
//     is enqueued without any host round trip.
//
// Arithmetic follows the reference's order and conjugation (alpha = <r,Ap>/<Ap,Ap> with conj on
// r, beta = <Ar,Aps_i>/<Aps_i,Aps_i> with conj on Ar: SURVEY.md §0 fact 2); the library is built
// with -ffp-contract=off so element-wise results round like the reference's.
#include <climits>
#include <cmath>
#include <type_traits>

#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "pw_tail_dev.h"

namespace mgcr {

static EnvSwitch g_lean{"MGCR_LEAN"};
bool set_lean_enabled(bool on) { return g_lean.set(on); }

// profile_spmv: hipEvents around the three phases of every iteration of the last profiled solve:
// 0 = alpha/r update (+ preconditioner), 1 = operator apply + beta dot products, 2 = direction build
static double g_prof_phase_ms[3] = {0., 0., 0.};
static int g_prof_iters = 0;
static int g_prof_fused = 0;   // 0: apply and dots separate; 1: one kernel; 2: + the direction build in that launch (gcr_stepbuild.hip); 3: + the next step's residual update; 4: the step that closes a cycle as well; 5: apply + dots in one kernel that also forms the residual update (gcr_fused.hip step_apply_xr*_kernel), build separate
void gcr_last_profile(double *phase_ms_total, int *n_iter, int *fused) {
    for (int k = 0; k < 3; k++) phase_ms_total[k] = g_prof_phase_ms[k];
    *n_iter = g_prof_iters;
    *fused = g_prof_fused;
}

struct GcrState {
    Op *A = nullptr;
    mgcr_gcr_param p{};
    int x0_mode = 1;
    std::vector<const cplx *> r_after;  // r_after[k]: where step k of the last solve left its residual (empty: not tracked)
    bool keep_pending = false;      // solves that only ever assign x (assign_x below) leave that to the caller: gcr_take_pending
    bool has_pending = false;
    PendingX pending{};
    bool defer_residual = false;    // nested: the caller forms the last step's residual itself (ResidualSel: r_prev - alpha ap)
    const cplx *defer_r_prev = nullptr, *defer_ap = nullptr, *defer_alpha = nullptr;
    int defer_it = 0;
    bool discard_residual = false;  // nested solves whose caller only wants x (post-smoother, coarsest solve): see alpha_only_kernel
    bool x_from_zero = false;  // next gcr_run: x0 = 0 and x's content is garbage (gcr_run_from_zero)
    int64_t n = 0;
    int storage = 0, restart = 0;
    std::vector<cplx *> ps, aps;
    cplx *r = nullptr, *ar = nullptr, *z = nullptr, *tmp = nullptr, *accp = nullptr, *accap = nullptr;
    cplx *x0 = nullptr;
    cplx *res_ring = nullptr;   // gcr_resident.hip
    cplx *xbak = nullptr;       // copy of the caller's x while a one-launch path may have to be abandoned (gcr_run)
    int64_t xbak_n = 0;
    DevState *st = nullptr;
    double *partsA = nullptr, *partsR = nullptr, *partsN = nullptr, *partsB = nullptr;
    // |b|^2 between the two smoothers of a V-cycle level (csrc/mg.hip): both get the same right-hand side, the kernels that embed the
    // apply sum |b|^2 over the same rows in the same order — the post-smoother folds the partials the pre-smoother's pass left
    // (partsN_of: the vector they belong to, nullptr = none; partsN_g: how many) instead of streaming b once more
    GcrState *bnorm_src = nullptr;
    const cplx *partsN_of = nullptr;
    int partsN_g = 0;
    cplx *den = nullptr;  // cached <Aps[i],Aps[i]> per slot
    double *hist = nullptr;
    int hist_cap = 0;
    int partsB_dirs = 0;
    // multi-GPU: folded scalars that are all-reduced over the ranks
    double *dA = nullptr;   // [4]
    double *dRB = nullptr;  // [1 + 2 * dirs]: |r|^2, then the beta numerators
    double *dN = nullptr;   // [2]: |b|^2, |r0|^2
    cplx *alphas = nullptr; // [storage]: alpha of the deferred x updates of the current restart cycle
    LeanCoef *lc = nullptr;
    // captured restart cycle (gcr_capture_cycle)
    hipGraphExec_t graph_exec = nullptr;
    const cplx *graph_x = nullptr;
    int graph_R = 0;
    int64_t graph_n = 0;
};

constexpr int64_t GRAPH_MAX_ROWS = 1 << 18;

static EnvSwitch g_bnorm_reuse{"MGCR_BNORM_REUSE"}, g_fuse_init{"MGCR_FUSE_INIT"}, g_skip_dead_ap{"MGCR_SKIP_DEAD_AP"};
static EnvSwitch g_stepbuild_xr{"MGCR_STEPBUILD_XR"}, g_stepbuild_close{"MGCR_STEPBUILD_CLOSE"};
// opt-in (MGCR_GRAPH=1 / mgcr_set_option("graph_replay")): see the measurements at gcr_capture_cycle
static EnvSwitch g_graph{"MGCR_GRAPH", false};
bool set_graph_enabled(bool on) { return g_graph.set(on); }

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
#define GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ void reset_kernel(DevState *st, const int *inherit, int inherit_it, double tol2) {
    st->stop_at = (inherit && inherit[0] < inherit[1] + inherit_it) ? -1 : INT_MAX;  // an outer solve that is over silences this one
    st->base = 0;
    st->iter = 0;
    st->npend = 0;
    st->bnorm2 = 0.;
    st->rr = 0.;
    st->tol2 = tol2;
    st->closed = 0;
}


// partials of |a|^2 -> parts[blk]
__global__ void __launch_bounds__(RED_THREADS) norm_partials_kernel(const cplx *__restrict__ a, int64_t n,
                                                                   double *__restrict__ parts, const DevState *st, int it) {
    __shared__ double lds[17];
    if (st && st->stop_at < st->base + it) return;
    double v[1] = {0.};
    GRID_STRIDE(i, n) {
        cplx t = a[i];
        v[0] += t.x * t.x + t.y * t.y;  // Re(conj(a) a), src/Fields.h:228-235
    }
    const double tot = block_sum_owner<1>(v, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = tot;
}

// partials of <r,Ap> (conj on r) and <Ap,Ap>  ->  partsA[0..3][blk]
__global__ void __launch_bounds__(RED_THREADS) dot2_partials_kernel(const cplx *__restrict__ r, const cplx *__restrict__ ap,
                                                                   int64_t n, double *__restrict__ parts, const DevState *st, int it) {
    __shared__ double lds[4 * 17];
    if (st->stop_at < st->base + it) return;
    double v[4] = {0., 0., 0., 0.};
    GRID_STRIDE(i, n) {
        cplx a = ap[i];
        cplx t = cconj_mul(r[i], a);
        v[0] += t.x; v[1] += t.y;
        cplx u = cconj_mul(a, a);
        v[2] += u.x; v[3] += u.y;
    }
    const double tot = block_sum_owner<4>(v, lds);
    if (threadIdx.x < 4) parts[threadIdx.x * RED_MAX_BLOCKS + blockIdx.x] = tot;
}

// |r|^2 (written twice: it is |b|^2 as well when r0 = b), <r,Ap> and <Ap,Ap> in one pass; same sums, in the
// same order, as norm_partials_kernel + dot2_partials_kernel
__global__ void __launch_bounds__(RED_THREADS) init3_partials_kernel(const cplx *__restrict__ r, const cplx *__restrict__ ap,
                                                                    int64_t n, double *__restrict__ partsN,
                                                                    double *__restrict__ partsR, double *__restrict__ partsA,
                                                                    const DevState *st, int it) {
    __shared__ double lds[5 * 17];
    if (st->stop_at < st->base + it) return;  // partsN == nullptr: r is not b (use_x0), |b|^2 is taken separately
    double v[5] = {0., 0., 0., 0., 0.};
    GRID_STRIDE(i, n) {
        cplx rv = r[i], a = ap[i];
        v[4] += rv.x * rv.x + rv.y * rv.y;
        cplx t = cconj_mul(rv, a);
        v[0] += t.x; v[1] += t.y;
        cplx u = cconj_mul(a, a);
        v[2] += u.x; v[3] += u.y;
    }
    const double tot = block_sum_owner<5>(v, lds);
    if (threadIdx.x < 4) partsA[threadIdx.x * RED_MAX_BLOCKS + blockIdx.x] = tot;
    if (threadIdx.x == 4) {
        partsR[blockIdx.x] = tot;
        if (partsN) partsN[blockIdx.x] = tot;
    }
}

// step 0 bookkeeping (src/GCR.h:213-216)
__global__ void __launch_bounds__(RED_THREADS) init_kernel(DevState *st, const double *__restrict__ partsN, int nblkN,
                                                           int strideN, const double *__restrict__ partsR, int nblkR,
                                                           int strideR, double *__restrict__ hist) {
    __shared__ double lds[17];
    if (st->stop_at < 0) return;
    double b[1], r[1];
    fold_partials<1>(partsN, nblkN, strideN, b, lds);
    fold_partials<1>(partsR, nblkR, strideR, r, lds);
    if (threadIdx.x == 0) {
        st->bnorm2 = b[0];
        st->rr = r[0];
        hist[0] = sqrt(r[0]) / sqrt(b[0]);
    }
}

// alpha = <r,Ap>/<Ap,Ap>;  x = x + p*alpha;  r = r - Ap*alpha  (src/GCR.h:230-233) + |r|^2 partials.
// DEFER (restart mode): x is not touched here; alpha is parked in alphas[slot] and the pending
// updates x += alpha_j p_j of a whole restart cycle are applied, in iteration order, by the
// build_kernel that closes the cycle (which streams those p_j anyway) or by flush_x_kernel at the
// end of the solve — 3 V less traffic per iteration, bit-identical x.
template <bool DEFER, bool LEAN>
__global__ void __launch_bounds__(RED_THREADS) xr_update_kernel(DevState *__restrict__ st, int it, const double *__restrict__ partsA,
                                                                int nblkA, int strideA, const cplx *__restrict__ p,
                                                                const cplx *__restrict__ ap, cplx *__restrict__ x,
                                                                const cplx *r_in, cplx *r_out, int64_t n, double *__restrict__ partsR,
                                                                cplx *__restrict__ den_slot, cplx *__restrict__ alphas, int slot,
                                                                LeanCoef *__restrict__ lc) {
    __shared__ double lds[4 * 17];
    if (st->stop_at < st->base + it) return;
    // the first trip's operands are requested BEFORE alpha is folded from the partials: one memory round trip of the
    // kernel's prologue (partials -> alpha -> first loads) disappears behind the other
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    cplx r0 = make_double2(0., 0.), a0 = r0;
    if (i0 < n) { r0 = r_in[i0]; a0 = ap[i0]; }
    double s[4];
    fold_partials<4>(partsA, nblkA, strideA, s, lds);
    const cplx num = make_double2(s[0], s[1]), den = make_double2(s[2], s[3]);
    const cplx alpha = to_sgpr(cdiv(num, den));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *den_slot = den;
        if (DEFER) {
            st->npend = slot + 1;
            if (!LEAN) alphas[slot] = alpha;
        }
    }
    if (DEFER && LEAN && blockIdx.x == 0 && (int)threadIdx.x < LND) lean_pending_update(lc, slot, alpha, (int)threadIdx.x);
    double v[1] = {0.};
    GRID_STRIDE(i, n) {
        if (!DEFER) x[i] = cadd(x[i], cmul(alpha, p[i]));
        const bool first = i == i0;
        cplx rn = csub(first ? r0 : r_in[i], cmul(alpha, first ? a0 : ap[i]));
        r_out[i] = rn;  // LEAN: the residual ring (r_out != r_in inside a cycle); else in place
        v[0] += rn.x * rn.x + rn.y * rn.y;
    }
    const double tot = block_sum_owner<1>(v, lds);
    if (threadIdx.x == 0) partsR[blockIdx.x] = tot;
}

// applies the x updates still pending when the solve ends (never skipped).  The usual counts (a smoother's 2-3 sweeps, up to a
// restart-5 cycle) get their loads issued together; same sums, same order.
template <int NP>
__device__ __forceinline__ void flush_x_rows(const cplx *__restrict__ alphas, const cplx *p0, const DirPtrs &d0, cplx *__restrict__ x, int64_t n,
                                             int assign) {
    cplx al[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) al[j] = to_sgpr(alphas[j]);
    GRID_STRIDE(i, n) {
        cplx pv[NP];
#pragma unroll
        for (int j = 0; j < NP; j++) pv[j] = (j == 0 ? p0 : d0.ps[j])[i];
        cplx xv = assign ? make_double2(0., 0.) : x[i];   // assign: x0 = 0 was never materialised (SolvePlan::assign_x)
#pragma unroll
        for (int j = 0; j < NP; j++) xv = cadd(xv, cmul(al[j], pv[j]));
        x[i] = xv;
    }
}
// p0_first: where P0 lives until the solve's first cycle is closed (SolvePlan::start1: b itself), d0.ps[0] after that
__global__ void __launch_bounds__(RED_THREADS) flush_x_kernel(DevState *__restrict__ st, const cplx *__restrict__ alphas, DirPtrs d0,
                                                              cplx *__restrict__ x, int64_t n, int assign, const cplx *p0_first) {
    const int np = st->npend;
    if (np <= 0) return;   // (also when an outer solver's stop predicate turned this whole solve into a no-op)
    // (a pointer of its own: a kernel argument that is written to moves to scratch, and every d0.ps[j] with it)
    const cplx *p0 = (p0_first && !st->closed) ? p0_first : d0.ps[0];
    switch (np) {
        case 1: flush_x_rows<1>(alphas, p0, d0, x, n, assign); return;
        case 2: flush_x_rows<2>(alphas, p0, d0, x, n, assign); return;
        case 3: flush_x_rows<3>(alphas, p0, d0, x, n, assign); return;
        case 4: flush_x_rows<4>(alphas, p0, d0, x, n, assign); return;
        case 5: flush_x_rows<5>(alphas, p0, d0, x, n, assign); return;
        default: break;
    }
    GRID_STRIDE(i, n) {
        cplx xv = assign ? make_double2(0., 0.) : x[i];
        for (int j = 0; j < np && j < LND; j++) xv = cadd(xv, cmul(alphas[j], (j == 0 ? p0 : d0.ps[j])[i]));
        x[i] = xv;
    }
}
// r = p0 = rhs at the start of a solve (src/GCR.h:189-190): one read, two writes instead of two copies
__global__ void __launch_bounds__(RED_THREADS) copy2_kernel(cplx *__restrict__ a, cplx *__restrict__ b, const cplx *__restrict__ src, int64_t n,
                                                            const DevState *st) {
    if (st->stop_at < 0) return;
    GRID_STRIDE(i, n) {
        const cplx v = src[i];
        a[i] = v;
        b[i] = v;
    }
}
__global__ void clear_pending_kernel(DevState *st) { st->npend = 0; }
__global__ void advance_kernel(DevState *st, int by) { st->base += by; }

// <Ar, Aps[j]> for j < NDT (conj on Ar, src/GCR.h:258) -> partsB[(base+j)*2 + {0,1}][blk].
// NDT is a template parameter so that the (1 + NDT) * U loads of one trip are issued back to back
// with no branch between them: the kernel is latency-bound otherwise (a wave with a single 1-KiB
// load in flight cannot cover HBM latency, even at 32 waves per CU).
template <int NDT, int U>
__global__ void __launch_bounds__(RED_THREADS, (NDT <= 6 ? 8 : 4)) multidot_kernel(const DevState *__restrict__ st, int it, const cplx *__restrict__ ar,
                                                               DirPtrs d, int base, int64_t n, RowMap rm,
                                                               double *__restrict__ partsB) {
    __shared__ double lds[2 * NDT * 17];
    if (st->stop_at < st->base + it) return;
    double v[2 * NDT];
#pragma unroll
    for (int j = 0; j < 2 * NDT; j++) v[j] = 0.;
    // rows of this workgroup's threads: RowMap (gcr_dev.h), shared with gcr_fused.hip's step_apply_kernel so that
    // either kernel yields the same partial sums
    int64_t first, end, step;
    row_range(rm, (int)blockIdx.x, (int)gridDim.x, n, &first, &end, &step);
    for (int64_t i0 = first; i0 < end; i0 += step * U) {
        cplx a[U], b[U][NDT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t i = i0 + u * step;
            if (i < end) {
                a[u] = ar[i];
#pragma unroll
                for (int j = 0; j < NDT; j++) b[u][j] = ld_stream<NTS>(d.aps[j] + i);
            } else {
                a[u] = make_double2(0., 0.);
#pragma unroll
                for (int j = 0; j < NDT; j++) b[u][j] = make_double2(0., 0.);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx t = cconj_mul(a[u], b[u][j]);
                v[2 * j] += t.x;
                v[2 * j + 1] += t.y;
            }
        }
    }
    const double mine = block_sum_owner<2 * NDT>(v, lds);
    if (threadIdx.x < 2 * NDT) partsB[(size_t)(2 * base + threadIdx.x) * RED_MAX_BLOCKS + blockIdx.x] = mine;
}

// beta_j = <Ar,Aps_j>/<Aps_j,Aps_j>;  p_corr -= ps_j*beta_j;  Ap_corr -= Aps_j*beta_j  (src/GCR.h:257-262)
// FIRST: accumulators start at 0 (else read from accp/accap); LAST: p' = dir + p_corr, Ap' = Ar + Ap_corr
// are written to the ring slot (src/GCR.h:265-266,286-287) and <r,Ap'>, <Ap',Ap'> partials emitted.
// RDIR: r is a different vector from dir (flexible preconditioning) and has to be loaded as well.
// When `book` is set, workgroup 0 also closes the step (src/GCR.h:270-274,288): folds |r|^2, bumps
// the iteration counter, records the history entry and raises the convergence flag.  The flag only
// takes effect from the next kernel on, so this step's directions are still built, as in the
// reference.
// XUPD (closing step of a restart cycle, NDT == restart): also applies the cycle's deferred
// x += alpha_j ps_j, j ascending = iteration order.
template <int NDT, bool FIRST, bool LAST, bool RDIR, bool XUPD>
__global__ void __launch_bounds__(RED_THREADS) build_kernel(DevState *__restrict__ st, int it, const double *__restrict__ partsB,
                                                            int nblkB, int strideB, int book,
                                                            const double *__restrict__ partsR, int nblkR, int strideR,
                                                            double *__restrict__ hist, int hist_cap,
                                                            const cplx *__restrict__ den, DirPtrs d, int base,
                                                            const cplx *__restrict__ dir, const cplx *__restrict__ r,
                                                            const cplx *__restrict__ ar, cplx *accp, cplx *accap,
                                                            cplx *p_out, cplx *ap_out, int64_t n,
                                                            double *__restrict__ partsA, cplx *__restrict__ x,
                                                            const cplx *__restrict__ alphas) {
    __shared__ double lds[2 * NDT * 17 > 4 * 17 ? 2 * NDT * 17 : 4 * 17];
    __shared__ cplx sbeta[NDT];
    if (st->stop_at < st->base + it) return;
    double s[2 * NDT];
    fold_partials<2 * NDT>(partsB + (size_t)(2 * base) * strideB, nblkB, strideB, s, lds);
    if (book && blockIdx.x == 0) {
        double rr[1];
        fold_partials<1>(partsR, nblkR, strideR, rr, lds);
        if (threadIdx.x == 0) {
            const int git = st->base + it;  // global_count
            st->iter = git;
            st->rr = rr[0];
            if (git < hist_cap) hist[git] = sqrt(rr[0]) / sqrt(st->bnorm2);
            // continue while |r|^2/|b|^2 > tol^2 (src/GCR.h:288); NaN compares false -> stop, like the reference
            if (gcr_solve_ends(rr[0], st->bnorm2, st->tol2)) st->stop_at = git;
            if (XUPD) st->npend = 0;
        }
    }
    if (threadIdx.x < NDT) {
        // s[] is identical in every thread; pick this thread's pair without dynamic register indexing
        cplx num = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++)
            if (j == (int)threadIdx.x) num = make_double2(s[2 * j], s[2 * j + 1]);
        sbeta[threadIdx.x] = cdiv(num, den[d.slot[threadIdx.x]]);
    }
    __syncthreads();
    cplx beta[NDT], alf[NDT];
#pragma unroll
    for (int j = 0; j < NDT; j++) {
        beta[j] = to_sgpr(sbeta[j]);
        alf[j] = XUPD ? to_sgpr(alphas[j]) : make_double2(0., 0.);
    }
    double v[4] = {0., 0., 0., 0.};
    GRID_STRIDE(i, n) {
        // all loads of the trip first, no branches in between
        cplx pj[NDT], aj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            pj[j] = ld_stream<NTS>(d.ps[j] + i);
            aj[j] = ld_stream<NTS>(d.aps[j] + i);
        }
        cplx pc = FIRST ? make_double2(0., 0.) : accp[i];
        cplx ac = FIRST ? make_double2(0., 0.) : accap[i];
        cplx dv = make_double2(0., 0.), av = make_double2(0., 0.), rv = make_double2(0., 0.);
        if (LAST) {
            dv = dir[i];
            av = ar[i];
            rv = RDIR ? r[i] : dv;
        }
        if (XUPD) {
            cplx xv = x[i];
#pragma unroll
            for (int j = 0; j < NDT; j++) xv = cadd(xv, cmul(alf[j], pj[j]));
            x[i] = xv;
        }
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            pc = csub(pc, cmul(beta[j], pj[j]));
            ac = csub(ac, cmul(beta[j], aj[j]));
        }
        if (LAST) {
            cplx pn = cadd(dv, pc);
            cplx an = cadd(av, ac);
            st_stream<NTS>(p_out + i, pn);  // p is next read as an "old slot"; Ap' is read by the very next kernel
            ap_out[i] = an;
            cplx t = cconj_mul(rv, an);
            v[0] += t.x; v[1] += t.y;
            cplx u = cconj_mul(an, an);
            v[2] += u.x; v[3] += u.y;
        } else {
            accp[i] = pc;
            accap[i] = ac;
        }
    }
    if (LAST) {
        const double mine = block_sum_owner<4>(v, lds);
        if (threadIdx.x < 4) partsA[threadIdx.x * RED_MAX_BLOCKS + blockIdx.x] = mine;
    }
}

// The last step of a nested solve whose caller only wants x (V-cycle post-smoother, coarsest solve): alpha and the
// pending-x bookkeeping of xr_update_kernel<true, true>, without its pass over r and Ap — nobody reads that residual.
__global__ void __launch_bounds__(RED_THREADS) alpha_only_kernel(DevState *st, int it, const double *__restrict__ partsA, int nblkA,
                                                                 int strideA, cplx *__restrict__ den_slot, int slot,
                                                                 LeanCoef *__restrict__ lc, cplx *__restrict__ alpha_out) {
    __shared__ double lds[4 * 17];
    if (st->stop_at < st->base + it) return;
    double s[4];
    fold_partials<4>(partsA, nblkA, strideA, s, lds);
    const cplx num = make_double2(s[0], s[1]), den = make_double2(s[2], s[3]);
    const cplx alpha = to_sgpr(cdiv(num, den));
    if (threadIdx.x == 0) {
        *den_slot = den;
        st->npend = slot + 1;
        st->iter = st->base + it;
        if (alpha_out) *alpha_out = alpha;
    }
    if ((int)threadIdx.x < LND) lean_pending_update(lc, slot, alpha, (int)threadIdx.x);
}

// Bookkeeping of a step without the direction build (src/GCR.h:270-274,288): the LAST iteration a solve can run
// (count == max_iter) still updates x and r and records |r|, but the next search direction the reference goes on to
// build (src/GCR.h:236-287: M r, A r, the beta dots, p, Ap) is never used — gcr_step's step_finish ends the step with this kernel.
__global__ void __launch_bounds__(RED_THREADS) finish_step_kernel(DevState *st, int it, const double *__restrict__ partsR, int nblkR,
                                                                  int strideR, double *__restrict__ hist, int hist_cap) {
    __shared__ double lds[17];
    if (st->stop_at < st->base + it) return;
    double rr[1];
    fold_partials<1>(partsR, nblkR, strideR, rr, lds);
    if (threadIdx.x == 0) close_step(st, it, rr[0], hist, hist_cap, false);
}

// LEAN, inside a restart cycle: direction k = NDT is started from D_k (the residual, or M r) and only
// its image is formed:  Ap_k = Ar - sum_{j<k} beta_j Ap_j  (same order as build_kernel), with the
// <r,Ap_k>, <Ap_k,Ap_k> partials; workgroup 0 extends the coefficient table by row k:
//   p_k = D_k - sum_j beta_j p_j   =>   t_k = -sum_j beta_j t_j ,  T_km = -sum_{j>=m} beta_j T_jm ,  T_kk = 1.
// (second launch bound: up to NDT = 5 the kernel fits 64 VGPRs, i.e. two 1024-thread workgroups per CU; left
// alone the compiler takes 84 for NDT = 4 and halves the residency: 48.4 us against 42 us at 128^3)
// PW (multi-GPU, peer-write scalars): the last workgroup folds the <r,Ap'>, <Ap',Ap'> partials and sums them over the ranks (pw_tail_dev.h)
template <int NDT, bool PW = false>
__global__ void __launch_bounds__(RED_THREADS, (NDT <= 5 ? 8 : 4)) build_lean_kernel(DevState *__restrict__ st, int it, const double *__restrict__ partsB,
                                                                 int nblkB, int strideB, const double *__restrict__ partsR, int nblkR,
                                                                 int strideR, double *__restrict__ hist, int hist_cap,
                                                                 const cplx *__restrict__ den, DirPtrs d, const cplx *__restrict__ r,
                                                                 const cplx *__restrict__ ar, cplx *ap_out, int64_t n,
                                                                 double *__restrict__ partsA, LeanCoef *__restrict__ lc, int closing, PwTail pw) {
    __shared__ double lds[2 * NDT * 17 > 4 * 17 ? 2 * NDT * 17 : 4 * 17];
    __shared__ cplx sbeta[NDT];
    if (st->stop_at < st->base + it) {
        if (PW) pw_tail(pw, (int)gridDim.x);   // a stopped solve: nothing to do, but the ranks' exchanges stay in lockstep (gcr_fused.hip step_apply_kernel)
        return;
    }
    double s[2 * NDT];
    fold_partials<2 * NDT>(partsB, nblkB, strideB, s, lds);
    if (blockIdx.x == 0) {
        double rr[1];
        fold_partials<1>(partsR, nblkR, strideR, rr, lds);
        if (threadIdx.x == 0) close_step(st, it, rr[0], hist, hist_cap, closing != 0);
    }
    if (threadIdx.x < NDT) {
        cplx num = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++)
            if (j == (int)threadIdx.x) num = make_double2(s[2 * j], s[2 * j + 1]);
        sbeta[threadIdx.x] = cdiv(num, den[d.slot[threadIdx.x]]);
    }
    __syncthreads();
    // closing (restart > 8: the cycle-closing step is close_x_kernel + this kernel with NDT = restart, writing
    // Ap_0' over slot 0 in place): no table row — the next cycle starts a new table
    if constexpr (NDT < LND)   // NDT == LND only ever runs as the closing step of a restart-16 cycle
    if (!closing && blockIdx.x == 0 && (int)threadIdx.x <= NDT) lean_table_row<NDT>(lc, sbeta, (int)threadIdx.x);   // row k = NDT
    cplx beta[NDT];
#pragma unroll
    for (int j = 0; j < NDT; j++) beta[j] = to_sgpr(sbeta[j]);
    double v[4] = {0., 0., 0., 0.};
    GRID_STRIDE(i, n) {
        cplx aj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) aj[j] = ld_stream<NTS>(d.aps[j] + i);
        const cplx av = ar[i], rv = r[i];
        cplx ac = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++) ac = csub(ac, cmul(beta[j], aj[j]));
        const cplx an = cadd(av, ac);
        if (ap_out) ap_out[i] = an;   // (nullptr: only <r,Ap_k>, <Ap_k,Ap_k> are wanted — the solve's last step follows and its caller discards the residual)
        cplx t = cconj_mul(rv, an);
        v[0] += t.x; v[1] += t.y;
        cplx u = cconj_mul(an, an);
        v[2] += u.x; v[3] += u.y;
    }
    const double mine = block_sum_owner<4>(v, lds);
    if (threadIdx.x < 4) partsA[threadIdx.x * RED_MAX_BLOCKS + blockIdx.x] = mine;
    if (PW) pw_tail(pw, (int)gridDim.x);
}

// LEAN, restart > 8: the x / P0 half of the cycle-closing step (the Ap half is build_lean_kernel with
// closing = 1).  Same sums, in the same order, as build_close_kernel; the 2 * NDT coefficients stay in LDS.
// Launched with RED_THREADS / 2 threads per workgroup (256 VGPRs each: 16 direction loads in flight plus the
// coefficients the compiler hoists out of the loop do not fit 128); it produces no partial sums, and
// fold_partials only needs blockDim >= the number of partials (<= RED_MAX_BLOCKS = RED_THREADS / 2).
template <int NDT>
__global__ void __launch_bounds__(RED_THREADS / 2) close_x_kernel(DevState *__restrict__ st, int it, const double *__restrict__ partsB,
                                                              int nblkB, int strideB, const cplx *__restrict__ den, DirPtrs d,
                                                              const cplx *__restrict__ dir, cplx *p_out, int64_t n,
                                                              cplx *__restrict__ x, const LeanCoef *__restrict__ lc) {
    __shared__ double lds[2 * NDT * 17];
    __shared__ cplx sbeta[NDT], scp[NDT], scx[NDT];
    if (st->stop_at < st->base + it) return;
    double s[2 * NDT];
    fold_partials<2 * NDT>(partsB, nblkB, strideB, s, lds);
    if (threadIdx.x < NDT) {
        cplx num = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++)
            if (j == (int)threadIdx.x) num = make_double2(s[2 * j], s[2 * j + 1]);
        sbeta[threadIdx.x] = cdiv(num, den[d.slot[threadIdx.x]]);
    }
    __syncthreads();
    if (threadIdx.x < NDT) {
        const int m = threadIdx.x;
        scp[m] = lean_close_coef(lc, sbeta, NDT, m);
        scx[m] = lc->cx[m];
    }
    __syncthreads();
    GRID_STRIDE(i, n) {
        cplx pj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) pj[j] = ld_stream<NTS>(d.ps[j] + i);
        const cplx dv = dir[i];
        cplx xv = x[i];
#pragma unroll
        for (int j = 0; j < NDT; j++) xv = cadd(xv, cmul(scx[j], pj[j]));
        x[i] = xv;
        cplx pc = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++) pc = csub(pc, cmul(scp[j], pj[j]));
        st_stream<NTS>(p_out + i, cadd(dv, pc));
    }
}

// LEAN, the step that closes a restart cycle (NDT = restart = lim).  d.ps[0] is P0, d.ps[m] the D_m;
// `dir` is D_R, what the new direction is started from.  In one pass:
//   x    += cx_0 P0 + sum_m cx_m D_m                        (the cycle's x updates, = sum_k alpha_k p_k)
//   P0'   = dir - cp_0 P0 - sum_m cp_m D_m                   (= dir - sum_j beta_j p_j, src/GCR.h:257-266)
//   Ap_0' = Ar - sum_j beta_j Ap_j                           with cp_m = sum_{j>=m} beta_j T_jm, cp_0 = sum_j beta_j t_j
// written in place over slot 0, plus the <r,Ap'>, <Ap',Ap'> partials and the step's bookkeeping.
template <int NDT, bool RDIR, bool PW = false>
__global__ void __launch_bounds__(RED_THREADS, (NDT <= 2 ? 8 : 4)) build_close_kernel(DevState *__restrict__ st, int it, const double *__restrict__ partsB,
                                                                  int nblkB, int strideB, const double *__restrict__ partsR, int nblkR,
                                                                  int strideR, double *__restrict__ hist, int hist_cap,
                                                                  const cplx *__restrict__ den, DirPtrs d, const cplx *__restrict__ dir,
                                                                  const cplx *__restrict__ r, const cplx *__restrict__ ar, cplx *p_out,
                                                                  cplx *ap_out, int64_t n, double *__restrict__ partsA,
                                                                  cplx *__restrict__ x, const LeanCoef *__restrict__ lc, PwTail pw) {
    __shared__ double lds[2 * NDT * 17 > 4 * 17 ? 2 * NDT * 17 : 4 * 17];
    __shared__ cplx sbeta[NDT], scp[NDT];
    if (st->stop_at < st->base + it) {
        if (PW) pw_tail(pw, (int)gridDim.x);   // (see build_lean_kernel)
        return;
    }
    double s[2 * NDT];
    fold_partials<2 * NDT>(partsB, nblkB, strideB, s, lds);
    if (blockIdx.x == 0) {
        double rr[1];
        fold_partials<1>(partsR, nblkR, strideR, rr, lds);
        if (threadIdx.x == 0) close_step(st, it, rr[0], hist, hist_cap, true);
    }
    if (threadIdx.x < NDT) {
        cplx num = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++)
            if (j == (int)threadIdx.x) num = make_double2(s[2 * j], s[2 * j + 1]);
        sbeta[threadIdx.x] = cdiv(num, den[d.slot[threadIdx.x]]);
    }
    __syncthreads();
    if (threadIdx.x < NDT) {
        const int m = threadIdx.x;
        scp[m] = lean_close_coef(lc, sbeta, NDT, m);
    }
    __syncthreads();
    cplx beta[NDT], cp[NDT], cx[NDT];
#pragma unroll
    for (int j = 0; j < NDT; j++) {
        beta[j] = to_sgpr(sbeta[j]);
        cp[j] = to_sgpr(scp[j]);
        cx[j] = to_sgpr(lc->cx[j]);
    }
    double v[4] = {0., 0., 0., 0.};
    GRID_STRIDE(i, n) {
        cplx pj[NDT], aj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            pj[j] = ld_stream<NTS>(d.ps[j] + i);
            aj[j] = ld_stream<NTS>(d.aps[j] + i);
        }
        const cplx dv = dir[i], av = ar[i];
        const cplx rv = RDIR ? r[i] : dv;
        cplx xv = x[i];
#pragma unroll
        for (int j = 0; j < NDT; j++) xv = cadd(xv, cmul(cx[j], pj[j]));
        x[i] = xv;
        cplx pc = make_double2(0., 0.), ac = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            pc = csub(pc, cmul(cp[j], pj[j]));
            ac = csub(ac, cmul(beta[j], aj[j]));
        }
        const cplx pn = cadd(dv, pc), an = cadd(av, ac);
        st_stream<NTS>(p_out + i, pn);
        ap_out[i] = an;
        cplx t = cconj_mul(rv, an);
        v[0] += t.x; v[1] += t.y;
        cplx u = cconj_mul(an, an);
        v[2] += u.x; v[3] += u.y;
    }
    const double mine = block_sum_owner<4>(v, lds);
    if (threadIdx.x < 4) partsA[threadIdx.x * RED_MAX_BLOCKS + blockIdx.x] = mine;
    if (PW) pw_tail(pw, (int)gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------------
template <typename T>
static int dalloc(T **p, size_t count) {
    hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", sizeof(T) * count, hipGetErrorString(e));
        return MGCR_ERR_ALLOC;
    }
    return MGCR_OK;
}

int op_apply_raw(Op *op, const cplx *x, cplx *y, int64_t n) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    switch (op->kind) {
        case OP_CSR:
            MGCR_CHECK((op->dist ? op->csr.nrow : op->csr.ncol) == n, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
            return csr_apply(op->csr, x, y, false, make_double2(0., 0.), op->dist);
        case OP_DIRAC:
            MGCR_CHECK(op->base->csr.nrow == n && (op->base->dist || op->base->csr.ncol == n), MGCR_ERR_INVALID,
                       "DiracOp needs a square matrix matching the Field dimension");
            // assertm(k != 0., ...) src/Operator.h:571
            MGCR_CHECK(op->k.x != 0. || op->k.y != 0., MGCR_ERR_INVALID, "No k value supplied for Dirac Operator!");
            return csr_apply(op->base->csr, x, y, true, op->k, op->base->dist);
        case OP_BCSR:
            if (op->dist) {   // row block of a distributed HierarchicalSparse: halo exchange, then the blocks read x or the halo segment
                MGCR_CHECK((int64_t)op->bcsr.nbrow * op->bcsr.bs == n, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
                MGCR_TRY(dist_halo_begin(op->dist, x));
                MGCR_TRY(dist_halo_end(op->dist));
                return bcsr_apply(op->bcsr, x, y, dist_halo_ptr(op->dist), op->bcsr.nbrow);
            }
            MGCR_CHECK((int64_t)op->bcsr.nbcol * op->bcsr.bs == n, MGCR_ERR_INVALID,
                       "Sparse matrix dimension does not match Field dimension!");
            return bcsr_apply(op->bcsr, x, y);
        case OP_GCR:
            return gcr_apply_as_operator(op->gcr, x, y);
        case OP_MG:
            return mg_apply(op->mg, x, y);
        case OP_DIRAC_EO:   // the Schur complement on the even half: two launches (evenodd.hip)
            return eo_apply(op, x, y, n);
        case OP_GCR32:   // the fp32 inner solve (gcr32.hip)
            return gcr32_apply(op, x, y, n);
        case OP_DIRAC_MULTI:   // (reached through a preconditioner slot; the entry points refuse it themselves)
            set_error("a MultiDiracOp has one hopping parameter per column of a block and cannot be applied to a single Field");
            return MGCR_ERR_UNSUPPORTED;
        case OP_DIRAC_EO_MULTI:   // (likewise)
            set_error("a MultiEvenOddDiracOp has one hopping parameter per column of a block and cannot be applied to a single Field");
            return MGCR_ERR_UNSUPPORTED;
        default:
            set_error("operator kind %d cannot be applied", (int)op->kind);
            return MGCR_ERR_UNSUPPORTED;
    }
}

// r = b - op(x): one pass for a Sparse (the SpMV epilogue takes b), apply + subtract otherwise
__global__ void __launch_bounds__(RED_THREADS) resid_sub_kernel(cplx *r, const cplx *__restrict__ b, int64_t n,
                                                                const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;
    GRID_STRIDE(i, n) r[i] = csub(b[i], r[i]);
}
int op_residual_raw(Op *op, const cplx *x, const cplx *b, cplx *r, int64_t n) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    if (op->kind == OP_CSR && op->csr.nrow == n && (op->dist ? true : op->csr.ncol == n) && b != r)
        return csr_apply(op->csr, x, r, true, make_double2(1., 0.), op->dist, b);
    MGCR_TRY(op_apply_raw(op, x, r, n));
    const SkipRef sk = get_apply_skip();
    hipLaunchKernelGGL(resid_sub_kernel, dim3(red_grid(n)), dim3(RED_THREADS), 0, ctx().stream, r, b, n, sk.p, sk.it);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

static void gcr_free_vectors(GcrState *s) {
    if (s->graph_exec) { hipGraphExecDestroy(s->graph_exec); s->graph_exec = nullptr; }
    for (cplx *p : s->ps) hipFree(p);
    for (cplx *p : s->aps) hipFree(p);
    s->ps.clear(); s->aps.clear();
    hipFree(s->r); hipFree(s->ar); hipFree(s->z); hipFree(s->tmp); hipFree(s->accp); hipFree(s->accap);
    hipFree(s->den); hipFree(s->hist); hipFree(s->partsB); hipFree(s->dRB); hipFree(s->alphas); hipFree(s->res_ring);
    s->res_ring = nullptr;
    s->r = s->ar = s->z = s->tmp = s->accp = s->accap = nullptr;
    s->den = nullptr; s->hist = nullptr; s->partsB = nullptr; s->dRB = nullptr; s->alphas = nullptr;
    s->n = 0; s->partsB_dirs = 0; s->hist_cap = 0;
}

void gcr_state_destroy(GcrState *s) {
    if (!s) return;
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    gcr_free_vectors(s);
    hipFree(s->xbak);
    hipFree(s->x0); hipFree(s->st); hipFree(s->partsA); hipFree(s->partsR); hipFree(s->partsN);
    hipFree(s->dA); hipFree(s->dN); hipFree(s->lc);
    delete s;
}

int gcr_state_create(Op *A, const mgcr_gcr_param *p, int x0_mode, GcrState **out) {
    MGCR_CHECK(p, MGCR_ERR_INVALID, "null GCR parameters");
    // assertm(param->truncation==0 || param->restart==0, ...) src/GCR.h:165
    MGCR_CHECK(p->truncation == 0 || p->restart == 0, MGCR_ERR_INVALID, "Do not support concurrent restarting and truncation.");
    MGCR_CHECK(p->truncation >= 0 && p->restart >= 0 && p->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_REFUSE_GCR32(A, "GCR");
    MGCR_TRY(gcr32_slot_check(p, A));
    GcrState *s = new GcrState();
    s->A = A;
    s->p = *p;
    s->x0_mode = x0_mode;
    int rc = dalloc(&s->st, 1);
    if (rc == MGCR_OK) rc = dalloc(&s->partsA, 4 * RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = dalloc(&s->partsR, RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = dalloc(&s->partsN, RED_MAX_BLOCKS);
    if (rc == MGCR_OK) rc = dalloc(&s->dA, 4);
    if (rc == MGCR_OK) rc = dalloc(&s->dN, 2);
    if (rc == MGCR_OK) rc = dalloc(&s->lc, 1);
    if (rc != MGCR_OK) { gcr_state_destroy(s); return rc; }
    *out = s;
    return MGCR_OK;
}

void gcr_state_set_use_x0(GcrState *s, bool use_x0) { s->p.use_x0 = use_x0 ? 1 : 0; }

int gcr_state_set_param(GcrState *s, const mgcr_gcr_param *p) {
    MGCR_CHECK(p->truncation == 0 || p->restart == 0, MGCR_ERR_INVALID, "Do not support concurrent restarting and truncation.");
    MGCR_CHECK(p->truncation >= 0 && p->restart >= 0 && p->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_TRY(gcr32_slot_check(p, s->A));
    s->p = *p;
    return MGCR_OK;
}

int gcr_state_set_operator(GcrState *s, Op *A) {
    MGCR_REFUSE_GCR32(A, "GCR");
    MGCR_TRY(gcr32_slot_check(&s->p, A));
    s->A = A;
    return MGCR_OK;
}

int gcr_state_set_x0(GcrState *s, const cplx *x0, int64_t n) {
    if (s->x0) { hipStreamSynchronize(ctx().stream); hipFree(s->x0); s->x0 = nullptr; }
    if (!x0) return MGCR_OK;
    MGCR_TRY(dalloc(&s->x0, (size_t)n));
    MGCR_TRY(k_copy(s->x0, x0, n));
    return MGCR_OK;
}

static int ensure_slot(GcrState *s, int slot) {
    while ((int)s->ps.size() <= slot) {
        cplx *a = nullptr, *b = nullptr;
        MGCR_TRY(dalloc(&a, (size_t)s->n));
        s->ps.push_back(a);
        MGCR_TRY(dalloc(&b, (size_t)s->n));
        s->aps.push_back(b);
    }
    return MGCR_OK;
}

static int gcr_prepare(GcrState *s, int64_t n) {
    const mgcr_gcr_param &p = s->p;
    // mode selection, src/GCR.h:171-185
    int storage = p.max_iter, restart;
    if (p.truncation != 0) storage = p.truncation;
    if (p.restart != 0) { restart = p.restart; storage = restart; } else restart = p.max_iter;
    // a restart cycle longer than the whole solve never closes: iteration k writes slot k <= max_iter,
    // so max_iter + 1 slots behave exactly like `restart` slots (smoothers: 2 sweeps of GCR(10))
    if (p.restart != 0 && p.max_iter >= 1 && p.max_iter + 1 < storage) storage = p.max_iter + 1;
    if (storage < 1) storage = 1;
    if (restart < 1) restart = 1;
    bool precond = p.left_precond || p.right_precond;
    if (s->n != n || s->storage != storage) {
        if (ctx().ready) hipStreamSynchronize(ctx().stream);
        gcr_free_vectors(s);
        s->n = n;
        s->storage = storage;
        MGCR_TRY(dalloc(&s->r, (size_t)n));
        MGCR_TRY(dalloc(&s->ar, (size_t)n));
        MGCR_TRY(dalloc(&s->den, (size_t)storage));
        MGCR_TRY(dalloc(&s->alphas, (size_t)storage));
        int bd = storage < ND ? ND : (storage + ND - 1) / ND * ND;
        MGCR_TRY(dalloc(&s->partsB, (size_t)2 * bd * RED_MAX_BLOCKS));
        MGCR_HIP(hipMemsetAsync(s->partsB, 0, sizeof(double) * (size_t)2 * bd * RED_MAX_BLOCKS, ctx().stream));
        s->partsB_dirs = bd;
        MGCR_TRY(dalloc(&s->dRB, (size_t)1 + 2 * bd));
        MGCR_HIP(hipMemsetAsync(s->dRB, 0, sizeof(double) * ((size_t)1 + 2 * bd), ctx().stream));
    }
    s->restart = restart;
    {   // history buffer: grows with max_iter, everything else is kept across solves
        int cap = (p.max_iter > 0 ? p.max_iter : 1) + 1;
        if (cap > s->hist_cap) {
            if (s->hist) { hipStreamSynchronize(ctx().stream); hipFree(s->hist); s->hist = nullptr; }
            MGCR_TRY(dalloc(&s->hist, (size_t)cap));
            s->hist_cap = cap;
        }
    }
    if (precond && !s->tmp) MGCR_TRY(dalloc(&s->tmp, (size_t)n));
    if (p.flexible && p.right_precond && !s->z) MGCR_TRY(dalloc(&s->z, (size_t)n));
    if (storage > ND && !s->accp) {
        MGCR_TRY(dalloc(&s->accp, (size_t)n));
        MGCR_TRY(dalloc(&s->accap, (size_t)n));
    }
    // restart / truncated modes: all slots up front; full mode grows on demand
    int want = (p.truncation != 0 || p.restart != 0) ? storage : 1;
    MGCR_TRY(ensure_slot(s, want - 1));
    return MGCR_OK;
}

#define KLAUNCH(kernel, grid, ...)                                                                 \
    do {                                                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(RED_THREADS), 0, ctx().stream, __VA_ARGS__);   \
        MGCR_HIP(hipGetLastError());                                                               \
    } while (0)

struct SkipGuard {
    SkipRef prev;
    explicit SkipGuard(SkipRef f) : prev(get_apply_skip()) { set_apply_skip(f); }
    ~SkipGuard() { set_apply_skip(prev); }
};

struct RedRef {  // where a consumer finds a reduction: slab of per-workgroup partials, or folded + all-reduced scalars
    const double *p;
    int nblk, stride;
};

struct BuildArgs {
    int g, nd;
    bool first, last, rdir, xupd;
    DevState *st;
    int it, book, base, hist_cap;
    RedRef B, R;
    double *hist, *partsA;
    DirPtrs d;
    const cplx *den, *dir, *r, *ar, *alphas;
    cplx *accp, *accap, *p_out, *ap_out, *x;
    int64_t n;
};

// RDIR only exists for the chunk that reads r (LAST), XUPD only for a closing step of one chunk
static int launch_build(const BuildArgs &a) {
    return dispatch_nd<1, ND>(a.nd, [&](auto N) -> int {
        auto bk = [&](auto fi, auto la, auto rd, auto xu) -> int {
            KLAUNCH((build_kernel<decltype(N)::value, decltype(fi)::value, decltype(la)::value, decltype(rd)::value, decltype(xu)::value>), a.g,
                    a.st, a.it, a.B.p, a.B.nblk, a.B.stride, a.book, a.R.p, a.R.nblk, a.R.stride, a.hist, a.hist_cap, a.den, a.d, a.base,
                    a.dir, a.r, a.ar, a.accp, a.accap, a.p_out, a.ap_out, a.n, a.partsA, a.x, a.alphas);
            return MGCR_OK;
        };
        constexpr std::true_type T{};
        constexpr std::false_type F{};
        if (a.first && a.last) return a.xupd ? (a.rdir ? bk(T, T, T, T) : bk(T, T, F, T)) : (a.rdir ? bk(T, T, T, F) : bk(T, T, F, F));
        if (a.first) return bk(T, F, F, F);
        if (a.last) return a.rdir ? bk(F, T, T, F) : bk(F, T, F, F);
        return bk(F, F, F, F);
    });
}

// the ring slots first .. first + nd - 1 in the first `width` entries (the unused ones repeat slot `first`)
static void fill_dirs(DirPtrs &d, const GcrState *s, int first, int nd, int width) {
    for (int j = 0; j < width; j++) {
        const int sl = first + (j < nd ? j : 0);
        d.ps[j] = s->ps[sl]; d.aps[j] = s->aps[sl]; d.slot[j] = sl;
    }
}

struct LeanArgs {
    int g, nd;
    bool rdir;
    DevState *st;
    int it, hist_cap;
    RedRef B, R;
    double *hist, *partsA;
    DirPtrs d;
    const cplx *den, *dir, *r, *ar;
    cplx *p_out, *ap_out, *x;
    int64_t n;
    LeanCoef *lc;
    const PwTail *pw = nullptr;   // multi-GPU: the kernel's last workgroup folds partsA and sums it over the ranks (up to 8 directions)
};

template <int HI, bool PW>
static int launch_build_lean_upto(const LeanArgs &a, int closing) {
    return dispatch_nd<1, HI>(a.nd, [&](auto N) -> int {
        KLAUNCH((build_lean_kernel<decltype(N)::value, PW>), a.g, a.st, a.it, a.B.p, a.B.nblk, a.B.stride, a.R.p, a.R.nblk, a.R.stride,
                a.hist, a.hist_cap, a.den, a.d, a.r, a.ar, a.ap_out, a.n, a.partsA, a.lc, closing, PW ? *a.pw : PwTail{});
        return MGCR_OK;
    });
}
static int launch_build_lean(const LeanArgs &a, int closing) {
    return a.pw ? launch_build_lean_upto<ND, true>(a, closing) : launch_build_lean_upto<LND, false>(a, closing);
}

static int launch_close_x(const LeanArgs &a) {
    return dispatch_nd<ND + 1, LND>(a.nd, [&](auto N) -> int {
        hipLaunchKernelGGL((close_x_kernel<decltype(N)::value>), dim3(2 * a.g), dim3(RED_THREADS / 2), 0, ctx().stream, a.st, a.it, a.B.p,
                           a.B.nblk, a.B.stride, a.den, a.d, a.dir, a.p_out, a.n, a.x, (const LeanCoef *)a.lc);
        MGCR_HIP(hipGetLastError());
        return MGCR_OK;
    });
}

static int launch_build_close(const LeanArgs &a) {
    return dispatch_nd<1, ND>(a.nd, [&](auto N) -> int {
        return dispatch_bool(a.rdir, [&](auto R) -> int {
            return dispatch_bool(a.pw != nullptr, [&](auto P) -> int {
                constexpr bool PW = decltype(P)::value;
                KLAUNCH((build_close_kernel<decltype(N)::value, decltype(R)::value, PW>), a.g, a.st, a.it, a.B.p, a.B.nblk, a.B.stride,
                        a.R.p, a.R.nblk, a.R.stride, a.hist, a.hist_cap, a.den, a.d, a.dir, a.r, a.ar, a.p_out, a.ap_out, a.n, a.partsA,
                        a.x, (const LeanCoef *)a.lc, PW ? *a.pw : PwTail{});
                return MGCR_OK;
            });
        });
    });
}

// read back iteration count / history once the solve has been enqueued (not for nested solves)
static int gcr_finish(GcrState *s, double *hist, int hist_cap, int *n_iter, int *converged) {
    Context &c = ctx();
    const mgcr_gcr_param &p = s->p;
    MGCR_HIP(hipMemcpyAsync(c.h_mail, s->st, sizeof(DevState), hipMemcpyDeviceToHost, c.stream));
    MGCR_HIP(hipStreamSynchronize(c.stream));
    DevState hs = *(const DevState *)c.h_mail;
    int it = hs.iter;
    if (n_iter) *n_iter = it;
    if (converged) *converged = (it == p.max_iter) ? 0 : 1;  // src/GCR.h:294-298
    std::vector<double> hh((size_t)it + 1);
    MGCR_HIP(hipMemcpy(hh.data(), s->hist, sizeof(double) * ((size_t)it + 1), hipMemcpyDeviceToHost));
    if (hist)
        for (int i = 0; i <= it && i < hist_cap; i++) hist[i] = hh[i];
    if (p.verbose) {  // src/GCR.h:213-216,270-274,293-300
        for (int i = 0; i <= it; i++) printf("Step %d residual norm = %.10e\n", i, hh[i]);
        if (it == p.max_iter)
            printf("GCR did not converge after %d steps! Residual norm = %.10e\n", p.max_iter, hh[it]);
        else
            printf("GCR converged after %d steps. Residual norm=%.10e\n", it, hh[it]);
    }
    return MGCR_OK;
}

// Every path decision of one solve, taken once (gcr_plan) before anything is enqueued: which kernels gcr_start and gcr_step launch.
struct SolvePlan {
    const cplx *rhs; cplx *x; int64_t n;
    bool nested, from_zero;   // from_zero (gcr_run_from_zero): x has to be zeroed here, unless the solve only ever ASSIGNS x
    const Op *b0;      // the Sparse behind A (A itself or a DiracOp's base); nullptr: A is something else
    bool shift; cplx k;   // DiracOp: y = x - k A x
    // Reductions.  Single GPU: consumers fold the producers' per-workgroup partials themselves.
    // Multi-GPU: a one-workgroup fold writes the local sums, RCCL all-reduces them in place on the
    // compute stream, and consumers read the global scalars (stride 1, one "partial").
    Comm *comm; bool multi; int g;
    RowMap rmap;       // row -> workgroup map of the dot-product kernels (gcr_dev.h): depends on how far the operator's rows reach
    int max_it;        // do..while: at least one iteration
    // the whole solve in one launch: of one workgroup (gcr_small.hip); with at most one row per thread of the chip, vectors in registers (gcr_resident.hip)
    bool small, resident;
    bool flex;
    bool skip_tail;    // the literal r = M(r) of src/GCR.h:236-238 changes the residual that is recorded: that mode keeps the full last step
    // restart mode with all slots handled by one build launch: defer the x updates of a cycle ...
    // ... and without the literal hooks (which replace r itself) the cycle runs lean (up to LND slots): see the file header
    bool lean, defer;
    // A lean solve that ends before its first restart cycle closes (smoothers: 2 sweeps of GCR(10)) never
    // overwrites its first direction and never updates r in place (the residual ring takes the updates): P0
    // simply IS r0 — no copy — and from x0 = 0 r0 IS rhs, in which case |b|^2 = |r0|^2 comes out of the pass
    // that takes <r,Ap> and <Ap,Ap>.
    bool alias_p0, alias0;
    const cplx *p0;
    // From x0 = 0, a solve that never closes a restart cycle touches x exactly once: flush_x_kernel at the end adds the
    // pending updates.  That kernel can just as well WRITE x = sum alpha_j p_j: no zeroing pass before, no read of x then.
    bool assign_x;
    bool fuse_ok;      // operator apply fused with the beta dot products: Sparse / DiracOp in a one-thread-per-row layout (gcr_fused.hip)
    // even-odd preconditioned DiracOp (evenodd.hip): the general multi-kernel path on the plain row map — no one-launch solve, step or
    // start, no residual update inside the apply, no graph replay; schur_fuse: stage 2 of its apply takes the beta dot products
    bool schur, schur_fuse;
    // The plain start of a solve on a fusable Sparse / DiracOp (r0 = p0 = rhs: no x0, no preconditioner): r and p0 are
    // written by ONE kernel from one read of rhs, and Ap_0 = A rhs comes out of the pass that also takes <r0,Ap0>,
    // <Ap0,Ap0> and |r0|^2 = |b|^2 (gcr_fused.hip init_apply_kernel) — 3 launches instead of 6 and 6 V less traffic
    // per solve; same sums in the same order as the separate kernels (test_fused_apply_and_dots_same_bits).  Worth
    // ~45 us per solve, i.e. 2-3 % of a 20-iteration solve at 128^3.
    bool fuse_start;
    bool fuse_init;    // step 0 of a smoother-like solve on a fusable Sparse / DiracOp: Ap_0 and its dot products in one pass (gcr_fused.hip)
    bool xr_fuse;      // latency regime: the residual update runs inside the apply kernel (gcr_fused.hip step_apply_xr*_kernel)
    // ... and where the steps are one launch each (gcr_stepbuild.hip), that start is ONE launch too (start_build_kernel): Ap0 = A b, the
    // sums, |b|^2 / hist[0], alpha and step 1's residual update r1 = b - alpha Ap0.  r and P0 are not copied: cycle 1 reads b where it
    // read them, the closing step reads P0 from b and writes P0' to its slot, flush_x_kernel picks P0 by DevState::closed.  Every
    // closing step of the solve has to be a one-launch step then (that sets `closed`): restart <= 5 directions, all of them stored.
    bool start1;
    bool use_graph;    // replay a captured restart cycle (gcr_capture_cycle, gcr_loop)
};

static SolvePlan gcr_plan(const GcrState *s, const cplx *rhs, cplx *x, bool nested, bool from_zero) {
    const mgcr_gcr_param &p = s->p;
    const Op *A = s->A, *base = A->kind == OP_DIRAC ? A->base : A;
    SolvePlan pl{};
    pl.rhs = rhs; pl.x = x; pl.n = A->dim; pl.nested = nested; pl.from_zero = from_zero;
    pl.b0 = base && base->kind == OP_CSR ? base : nullptr;
    pl.shift = A->kind == OP_DIRAC; pl.k = A->k;
    pl.max_it = p.max_iter > 0 ? p.max_iter : 1;
    pl.flex = p.flexible && p.right_precond;
    pl.skip_tail = !p.right_precond || pl.flex;
    pl.schur = A->kind == OP_DIRAC_EO;
    pl.lean = p.restart != 0 && s->storage <= LND && g_lean.on() && !p.left_precond && (!p.right_precond || pl.flex);
    pl.small = gcr_small_eligible(A, p, s->storage, pl.n);
    const bool handoff = nested && (s->keep_pending || s->defer_residual);   // callers that take x or r in pieces (V-cycle pre-smoother)
    pl.resident = !pl.small && !g_graph.on() && gcr_resident_eligible(A, p, s->storage, s->restart, pl.n, pl.lean, handoff);
    if (pl.small || pl.resident) return pl;   // (one launch for the whole solve: nothing below is consulted)
    pl.comm = A->kind == OP_DIRAC ? A->base->comm : A->comm;
    pl.multi = comm_collectives(pl.comm);
    pl.g = red_grid(pl.n);
    pl.rmap = pl.schur ? RowMap{0, 0, 0, 0, 0, 0} : make_row_map(pl.n, pl.g, pl.b0 ? pl.b0->csr.reach : 0);
    pl.schur_fuse = pl.schur && !p.left_precond && eo_schur_fusable(A);
    pl.defer = pl.lean || (p.restart != 0 && s->storage <= ND);
    pl.alias_p0 = pl.lean && !pl.flex && p.max_iter >= 1 && p.max_iter < p.restart;
    pl.alias0 = pl.alias_p0 && !p.use_x0;
    pl.p0 = pl.alias0 ? rhs : pl.alias_p0 ? (const cplx *)s->r : (const cplx *)s->ps[0];
    pl.assign_x = from_zero && pl.alias_p0 && !p.use_x0;
    pl.fuse_ok = pl.b0 && !p.left_precond && csr_fusable(pl.b0->csr, pl.b0->dist) && pl.b0->csr.nrow == pl.n;
    pl.fuse_start = pl.fuse_ok && !pl.alias_p0 && !pl.flex && !p.use_x0 && !p.left_precond && !p.right_precond && g_fuse_init.on();
    pl.fuse_init = pl.fuse_ok && pl.alias_p0 && g_fuse_init.on();
    const bool xr_able = pl.fuse_ok && pl.lean && !pl.flex && s->restart > 1 && csr_xr_fusable(pl.b0->csr, pl.b0->dist);
    pl.xr_fuse = xr_able && !pl.multi;
    pl.start1 = pl.fuse_start && pl.lean && s->restart > 1 && s->restart <= 5 && s->storage >= s->restart &&
                pl.rmap.band == 0 && !g_graph.on() && g_stepbuild_close.on() &&
                !(nested && p.max_iter <= 1 && (s->defer_residual || s->discard_residual)) && !xr_able &&
                csr_start_build_eligible(pl.b0->csr, pl.b0->dist) && csr_step_build_eligible(pl.b0->csr, pl.b0->dist, s->restart);
    pl.use_graph = g_graph.on() && pl.n <= GRAPH_MAX_ROWS && pl.defer && !pl.multi && !p.left_precond && !p.right_precond &&
                   !p.profile_spmv && pl.max_it >= 2 * s->restart && s->restart <= s->storage && !pl.schur;
    return pl;
}

// What moves from step to step: the slot ring, where r and P0 live, and where consumers find the newest reductions
struct StepCursor {
    int iter_count = 0;   // steps into the current restart cycle
    int cur = 0;          // slot of the newest direction
    int global = 0;       // steps enqueued (or replayed) so far
    const cplx *rcur = nullptr;      // lean: where the current residual lives (s->r at the start of every cycle)
    const cplx *p0_live = nullptr;   // where the closing step reads P0 (start1: b until cycle 1 closes)
    bool xr_prefetched = false;      // the next iteration's residual update already ran at the end of this one's launch
    RedRef refA{}, refR{};
};

// profile_spmv: 4 events per iteration, around its three phases | xr (+M) | apply + dots | build |
struct PhaseMarks {
    bool on = false;
    std::vector<hipEvent_t> ev;
    size_t iter0 = 0;
    bool step_build = false, step_build_xr = false, step_build_close = false;   // one-launch steps seen (g_prof_fused)
    // phase k of the iteration begins (k = 3: the iteration ends); phases that were skipped get empty intervals
    int enter(int k) {
        if (k == 0) iter0 = ev.size();
        while (on && ev.size() < iter0 + (size_t)k + 1) {
            hipEvent_t e;
            MGCR_HIP(hipEventCreate(&e));
            MGCR_HIP(hipEventRecord(e, ctx().stream));
            ev.push_back(e);
        }
        return MGCR_OK;
    }
    int read_out(const SolvePlan &pl) {
        if (ev.empty()) return MGCR_OK;
        MGCR_HIP(hipStreamSynchronize(ctx().stream));
        for (int k = 0; k < 3; k++) g_prof_phase_ms[k] = 0.;
        for (size_t i = 0; i + 3 < ev.size(); i += 4)
            for (int k = 0; k < 3; k++) {
                float ms = 0.f;
                hipEventElapsedTime(&ms, ev[i + k], ev[i + k + 1]);
                g_prof_phase_ms[k] += ms;
            }
        g_prof_iters = (int)(ev.size() / 4);
        g_prof_fused = step_build_close ? 4 : step_build_xr ? 3 : step_build ? 2 : (pl.fuse_ok && pl.xr_fuse) ? 5 : pl.fuse_ok ? 1 : 0;
        for (hipEvent_t e : ev) hipEventDestroy(e);
        return MGCR_OK;
    }
};

// r = rhs (src/GCR.h:189); p = r (or M r); Ap = A p; both go straight into slot 0 (src/GCR.h:190-191,208-211); the literal hooks
static int start_vectors(GcrState *s, const SolvePlan &pl) {
    const mgcr_gcr_param &p = s->p;
    const int64_t n = pl.n;
    // the reference ignores x0 here unless use_x0 is requested
    if (p.use_x0) {
        MGCR_TRY(op_residual_raw(s->A, pl.x, pl.rhs, s->r, n));
    } else if (pl.start1) {
        // (r0 = P0 = rhs, read in place)
    } else if (pl.fuse_start) {
        KLAUNCH(copy2_kernel, pl.g, s->r, s->ps[0], pl.rhs, n, (const DevState *)s->st);
    } else if (!pl.alias0) {
        MGCR_TRY(k_copy(s->r, pl.rhs, n));
    }
    if (pl.flex) {
        MGCR_TRY(op_apply_raw((Op *)p.right_precond, s->r, s->z, n));
        MGCR_TRY(k_copy(s->ps[0], s->z, n));
    } else if (!pl.alias_p0 && !pl.fuse_start) {
        MGCR_TRY(k_copy(s->ps[0], s->r, n));
    }
    if (!pl.fuse_init && !pl.fuse_start) MGCR_TRY(op_apply_raw(s->A, pl.p0, s->aps[0], n));
    if (!pl.flex) {  // literal hooks, src/GCR.h:197-204 (after p and Ap were formed)
        if (p.right_precond) { MGCR_TRY(op_apply_raw((Op *)p.right_precond, s->r, s->tmp, n)); std::swap(s->r, s->tmp); }
        if (p.left_precond) { MGCR_TRY(op_apply_raw((Op *)p.left_precond, s->r, s->tmp, n)); std::swap(s->r, s->tmp); }
    }
    return MGCR_OK;
}

// |b|^2, |r0|^2, <r0,Ap0>, <Ap0,Ap0> in their five forms (the fused ones form Ap_0 as well); *normN: where |b|^2's partials are
static int start_partials(GcrState *s, const SolvePlan &pl, StepCursor &c, const double **normN) {
    const int64_t n = pl.n;
    const int g = pl.g;
    const cplx *rhs = pl.rhs, *none = nullptr;
    const DevState *cst = s->st;
    if (pl.start1) {
        const int nxt1 = 1 % s->storage;   // where step 1 leaves its residual (step_residual_lean: dslot)
        MGCR_TRY(ensure_slot(s, nxt1));
        MGCR_TRY(csr_start_build(pl.b0->csr, rhs, pl.shift, pl.k, s->aps[0], s->st, s->hist, s->lc, s->den, nxt1 >= 1 ? s->ps[nxt1] : s->r,
                                 s->partsR, pl.rmap));
        c.xr_prefetched = true;
    } else if (pl.fuse_start) {
        MGCR_TRY(csr_init_apply(pl.b0->csr, rhs, s->aps[0], pl.shift, pl.k, none, s->partsA, s->partsR, s->partsN, pl.b0->dist, pl.rmap));
    } else if (pl.fuse_init) {
        const GcrState *src = s->bnorm_src;
        double *partsN = s->partsN;
        if (!pl.alias0 && !pl.multi && src && src->partsN_of == rhs && src->partsN_g == g && g_bnorm_reuse.on()) {
            *normN = src->partsN;   // |b|^2: the partials of the solve that ran on this b just before
            partsN = nullptr;
        }
        MGCR_TRY(csr_init_apply(pl.b0->csr, pl.p0, s->aps[0], pl.shift, pl.k, (pl.alias0 || !partsN) ? none : rhs, s->partsA, s->partsR, partsN,
                                pl.b0->dist, pl.rmap));
        if (partsN) { s->partsN_of = rhs; s->partsN_g = g; }
    } else if (pl.alias0) {
        KLAUNCH(init3_partials_kernel, g, rhs, (const cplx *)s->aps[0], n, s->partsN, s->partsR, s->partsA, cst, 0);
    } else if (pl.alias_p0) {
        KLAUNCH(norm_partials_kernel, g, rhs, n, s->partsN, cst, 0);
        KLAUNCH(init3_partials_kernel, g, (const cplx *)s->r, (const cplx *)s->aps[0], n, (double *)nullptr, s->partsR, s->partsA, cst, 0);
    } else {
        KLAUNCH(norm_partials_kernel, g, rhs, n, s->partsN, cst, 0);
        KLAUNCH(norm_partials_kernel, g, (const cplx *)s->r, n, s->partsR, cst, 0);
        KLAUNCH(dot2_partials_kernel, g, (const cplx *)s->r, (const cplx *)s->aps[0], n, s->partsA, cst, 0);
    }
    return MGCR_OK;
}

// step 0: r, P0, Ap_0, the initial reductions and the step's bookkeeping; leaves the cursor at the first iteration
static int gcr_start(GcrState *s, const SolvePlan &pl, StepCursor &c) {
    const mgcr_gcr_param &p = s->p;
    const int g = pl.g;
    MGCR_TRY(start_vectors(s, pl));
    MGCR_CHECK(!pl.multi || (!p.left_precond && (!p.right_precond || pl.flex)), MGCR_ERR_UNSUPPORTED,
               "on a distributed operator only flexible right preconditioning is available (set flexible = 1)");
    const double *normN = s->partsN;
    MGCR_TRY(start_partials(s, pl, c, &normN));
    c.refA = {s->partsA, g, RED_MAX_BLOCKS};
    c.refR = {s->partsR, g, RED_MAX_BLOCKS};
    if (pl.multi) {
        MGCR_TRY(comm_fold_allreduce(pl.comm, s->partsN, 1, s->partsR, 1, s->dN, g));
        MGCR_TRY(comm_fold_allreduce(pl.comm, s->partsA, 4, nullptr, 0, s->dA, g));
        KLAUNCH(init_kernel, 1, s->st, (const double *)s->dN, 1, 1, (const double *)(s->dN + 1), 1, 1, s->hist);
        c.refA = {s->dA, 1, 1};
        c.refR = {s->dRB, 1, 1};
    } else if (!pl.start1) {
        KLAUNCH(init_kernel, 1, s->st, normN, g, RED_MAX_BLOCKS, (const double *)s->partsR, g, RED_MAX_BLOCKS, s->hist);
    }
    c.rcur = (pl.alias0 || pl.start1) ? pl.rhs : s->r;
    c.p0_live = pl.start1 ? pl.rhs : (const cplx *)s->ps[0];
    // where each step leaves the (true recurrence) residual — not with the literal hooks, which replace r by M r
    s->r_after.clear();
    if (!p.left_precond && (!p.right_precond || pl.flex) && pl.max_it <= LND) s->r_after.assign((size_t)pl.max_it + 1, nullptr);
    return MGCR_OK;
}

// One iteration's constants (from the cursor) and what its phases hand to each other
struct Step {
    int it;         // iteration number relative to DevState::base
    bool tail;      // the last iteration the solve can run, and nothing of the next direction is wanted (skip_tail)
    int lim;        // stored directions, src/GCR.h:251
    int ic_next;    // iter_count after this step (0: the step closes a restart cycle)
    int nxt;        // slot the new direction goes to (src/GCR.h:277-287)
    const cplx *dir = nullptr;     // what the new direction is started from: r, or M r
    bool xr_now = false;           // the residual update runs inside the apply kernel
    const cplx *xr_in = nullptr;   // ... from this residual
    bool ended = false;            // the residual update was all this step had to do (alpha_only_kernel)
};

// M r behind a step's residual update (flexible mode).  The step's stopping test comes only with its build, so this apply is
// enqueued whether or not the solve ends on r, and behind the last update its result is never used.  A low-precision GCR — an
// expensive apply — is handed the test itself (Gcr32Gate) and does not run then; every other operator is applied as before.
// (In flexible mode the update that precedes this is always xr_update_kernel, which leaves the step's |r|^2 partials in s->partsR:
// the residual update fused into an apply and the one-launch steps exclude a preconditioner.)
static int flex_precond_apply(GcrState *s, const SolvePlan &pl, cplx *out) {
    Op *M = (Op *)s->p.right_precond;
    if (M->kind == OP_GCR32 && !pl.multi)
        return gcr32_apply(M, s->r, out, pl.n, Gcr32Gate{s->partsR, pl.g, RED_MAX_BLOCKS, &s->st->bnorm2, &s->st->tol2});
    return op_apply_raw(M, s->r, out, pl.n);
}

// alpha, x, r of a lean step (r goes to the residual ring); with both endings of a nested solve whose caller does not want the last residual
static int step_residual_lean(GcrState *s, const SolvePlan &pl, StepCursor &c, Step &st) {
    const int cur = c.cur;
    // D_nxt, what direction nxt is started from, lands in the p slot of that direction (nxt >= 1);
    // the step that closes the cycle only needs it for its own build
    cplx *dslot = st.nxt >= 1 ? s->ps[st.nxt] : (pl.flex ? s->z : s->r);
    cplx *r_out = pl.flex ? s->r : dslot;
    const bool alpha_only = st.tail && pl.nested && !pl.multi;   // a nested solve's last step whose caller does not read its residual:
    const bool deferred = alpha_only && s->defer_residual && !pl.flex && !s->r_after.empty();   // ... it forms it itself (ResidualSel)
    if (deferred || (alpha_only && s->discard_residual)) {
        KLAUNCH(alpha_only_kernel, 1, s->st, st.it, c.refA.p, c.refA.nblk, c.refA.stride, s->den + cur, cur, s->lc,
                deferred ? s->alphas + cur : (cplx *)nullptr);
        if (deferred) {   // from the previous residual, Ap and alpha
            s->defer_r_prev = c.rcur; s->defer_ap = s->aps[cur]; s->defer_alpha = s->alphas + cur; s->defer_it = c.global;
            s->r_after[(size_t)c.global] = c.rcur;   // placeholder: never read (st->iter == defer_it takes the on-the-fly path)
        } else {
            s->r_after.clear();
        }
        st.ended = true;
        return MGCR_OK;
    }
    st.xr_now = pl.xr_fuse && !st.tail;
    st.xr_in = c.rcur;
    if (c.xr_prefetched) c.xr_prefetched = false;   // the previous step's launch ended with this update (gcr_stepbuild.hip)
    else if (!st.xr_now)
        KLAUNCH((xr_update_kernel<true, true>), pl.g, s->st, st.it, c.refA.p, c.refA.nblk, c.refA.stride, (const cplx *)nullptr,
                (const cplx *)s->aps[cur], pl.x, c.rcur, r_out, pl.n, s->partsR, s->den + cur, s->alphas, cur, s->lc);
    c.rcur = r_out;
    st.dir = r_out;
    if (pl.flex && !st.tail) {
        MGCR_TRY(flex_precond_apply(s, pl, dslot));
        st.dir = dslot;
    }
    return MGCR_OK;
}

// alpha, x, r of a classic step (r in place), and the preconditioner: flexible, or the literal hook
static int step_residual_classic(GcrState *s, const SolvePlan &pl, StepCursor &c, Step &st) {
    const mgcr_gcr_param &p = s->p;
    const int cur = c.cur;
    MGCR_TRY(dispatch_bool(pl.defer, [&](auto D) -> int {
        KLAUNCH((xr_update_kernel<decltype(D)::value, false>), pl.g, s->st, st.it, c.refA.p, c.refA.nblk, c.refA.stride,
                (const cplx *)s->ps[cur], (const cplx *)s->aps[cur], pl.x, (const cplx *)s->r, s->r, pl.n, s->partsR, s->den + cur, s->alphas,
                cur, s->lc);
        return MGCR_OK;
    }));
    st.dir = s->r;
    if (pl.flex && !st.tail) {
        MGCR_TRY(flex_precond_apply(s, pl, s->z));
        st.dir = s->z;
    } else if (p.right_precond && !pl.flex) {  // src/GCR.h:236-238
        MGCR_TRY(op_apply_raw((Op *)p.right_precond, s->r, s->tmp, pl.n));
        std::swap(s->r, s->tmp);
        st.dir = s->r;
        KLAUNCH(norm_partials_kernel, pl.g, (const cplx *)s->r, pl.n, s->partsR, (const DevState *)s->st, st.it);
    }
    return MGCR_OK;
}

// Nothing after the solve's last iteration: no preconditioner apply, no A r, no beta dots, no direction build — only the
// step's bookkeeping (the x updates still pending are applied by flush_x_kernel)
static int step_finish(GcrState *s, const SolvePlan &pl, const StepCursor &c, const Step &st) {
    RedRef fr = c.refR;
    if (pl.multi) {
        MGCR_TRY(comm_fold_allreduce(pl.comm, s->partsR, 1, nullptr, 0, s->dRB, pl.g));
        fr = {s->dRB, 1, 1};
    }
    KLAUNCH(finish_step_kernel, 1, s->st, st.it, fr.p, fr.nblk, fr.stride, s->hist, s->hist_cap);
    return MGCR_OK;
}

// apply + dots + build in ONE launch (gcr_stepbuild.hip) where A r of a thread's rows fits LDS; up to 5 directions the step
// that closes a cycle has its one-launch form too
static bool step_is_one_launch(const SolvePlan &pl, const Step &st) {
    return pl.fuse_ok && pl.lean && !pl.flex && !pl.multi && !st.xr_now && pl.rmap.band == 0 &&
           (st.ic_next != 0 || g_stepbuild_close.on()) && !g_graph.on() &&   // (a captured cycle would replay the exchange's generation numbers)
           csr_step_build_eligible(pl.b0->csr, pl.b0->dist, st.lim);
}
static int step_one_launch(GcrState *s, const SolvePlan &pl, StepCursor &c, PhaseMarks &marks, const Step &st) {
    const int lim = st.lim;
    const bool closes = st.ic_next == 0;   // (lim == restart then)
    const cplx *vecs[FND], *cps[FND];
    for (int j = 0; j < FND; j++) { vecs[j] = s->aps[j < lim ? j : 0]; cps[j] = j < lim && j > 0 ? s->ps[j] : c.p0_live; }
    // ... and, unless the next step is the solve's last (whose update takes other kernels), that step's residual update too:
    // r and the new Ap of a thread's rows are on the chip, alpha costs one more exchange instead of a launch
    cplx *xr_out = nullptr;
    const bool next_is_special_last = c.global + 1 == pl.max_it && pl.nested && (s->defer_residual || s->discard_residual);
    if (c.global + 1 <= pl.max_it && !next_is_special_last && g_stepbuild_xr.on()) {
        const int ic2 = ((st.ic_next + 1) % s->restart == 0) ? 0 : st.ic_next + 1;
        const int nxt2 = ic2 % s->storage;
        MGCR_TRY(ensure_slot(s, nxt2));
        xr_out = nxt2 >= 1 ? s->ps[nxt2] : s->r;
    }
    MGCR_TRY(csr_step_build(pl.b0->csr, st.dir, pl.shift, pl.k, vecs, lim, s->st, st.it, c.refR.p, c.refR.nblk, c.refR.stride, s->hist,
                            s->hist_cap, s->den, s->aps[st.nxt], s->partsA, s->lc, pl.rmap, xr_out, s->den + st.nxt, st.nxt, s->partsR,
                            closes ? cps : nullptr, closes ? s->ps[0] : nullptr, closes ? pl.x : nullptr));
    c.xr_prefetched = xr_out != nullptr;
    marks.step_build = true;
    marks.step_build_xr = marks.step_build_xr || c.xr_prefetched;
    marks.step_build_close = marks.step_build_close || closes;
    if (closes) c.p0_live = s->ps[0];
    return MGCR_OK;
}

// Ar = A dir (+ the literal left hook) and the <Ar, Aps_j> partials; *tail_rb: the fold + exchange of |r|^2 and the beta
// numerators ran inside the apply kernel
static int step_apply_dots(GcrState *s, const SolvePlan &pl, const StepCursor &c, const Step &st, bool *tail_rb) {
    const int lim = st.lim, nchunk = (lim + ND - 1) / ND;
    int ch0 = 0;
    if (pl.fuse_ok) {
        // Ar = A dir and the <Ar, Aps_j> partials of the first FND = 10 stored directions in one pass (gcr_fused.hip);
        // with more than that (restart > 10) multidot_kernel takes directions 8.. in its chunks of ND = 8 (8 and 9 twice:
        // the same sums, the same bits)
        const int nf = lim < FND ? lim : FND;
        const cplx *vecs[FND];
        for (int j = 0; j < FND; j++) vecs[j] = s->aps[j < nf ? j : 0];
        const CsrDev &M = pl.b0->csr;
        DistCsr *dist = pl.b0->dist;
        // multi-GPU, scalars by peer writes: the apply kernel's last workgroup folds |r|^2 (the residual update's partials)
        // and the beta numerators and sums them over the ranks — no fold + exchange launch behind it (pw_tail_dev.h)
        PwTail pw;
        if (st.xr_now) {
            MGCR_TRY(csr_step_apply_xr(M, st.xr_in, s->aps[c.cur], const_cast<cplx *>(st.dir), s->ar, pl.shift, pl.k, vecs, nf, s->partsB,
                                       s->partsR, s->st, st.it, c.refA.p, c.refA.nblk, c.refA.stride, s->den + c.cur, c.cur, s->lc, pl.rmap));
        } else {
            *tail_rb = pl.multi && lim <= FND && csr_step_apply_has_pw_tail(M, dist) && comm_pw_tail_begin(pl.comm, &pw);
            if (*tail_rb) { pw.pa = s->partsR; pw.na = 1; pw.pb = s->partsB; pw.nb = 2 * lim; pw.out = s->dRB; pw.nblk = pl.g; }
            MGCR_TRY(csr_step_apply(M, st.dir, s->ar, pl.shift, pl.k, vecs, nf, s->partsB, dist, pl.rmap, *tail_rb ? &pw : nullptr));
        }
        ch0 = lim <= FND ? nchunk : 1;
    } else if (pl.schur_fuse) {
        // t = D_oe dir, then Ar = dir - k^2 D_eo t with the partials of the first FND directions (evenodd.hip); the rest as above
        const int nf = lim < FND ? lim : FND;
        const cplx *vecs[FND];
        for (int j = 0; j < FND; j++) vecs[j] = s->aps[j < nf ? j : 0];
        MGCR_TRY(eo_schur_step(s->A, st.dir, s->ar, vecs, nf, s->partsB, pl.rmap));
        ch0 = lim <= FND ? nchunk : 1;
    } else {
        MGCR_TRY(op_apply_raw(s->A, st.dir, s->ar, pl.n));  // src/GCR.h:242
        if (s->p.left_precond) {                            // src/GCR.h:245-247
            MGCR_TRY(op_apply_raw((Op *)s->p.left_precond, s->ar, s->tmp, pl.n));
            std::swap(s->ar, s->tmp);
        }
    }
    for (int ch = ch0; ch < nchunk; ch++) {
        DirPtrs d;
        const int nd = lim - ch * ND < ND ? lim - ch * ND : ND;
        fill_dirs(d, s, ch * ND, nd, ND);
        MGCR_TRY((dispatch_nd<1, ND>(nd, [&](auto N) -> int {
            constexpr int NDT = decltype(N)::value;
            KLAUNCH((multidot_kernel<NDT, (NDT <= 2 ? 2 : 1)>), pl.g, (const DevState *)s->st, st.it, (const cplx *)s->ar, d, ch * ND, pl.n,
                    pl.rmap, s->partsB);
            return MGCR_OK;
        })));
    }
    return MGCR_OK;
}

// the lean build: inside a cycle (build_lean_kernel), or closing it in one kernel or, with restart > 8, in two;
// *tail_a: the build kernel folded and exchanged <r,Ap'>, <Ap',Ap'> itself
static int step_build_lean(GcrState *s, const SolvePlan &pl, const StepCursor &c, const Step &st, RedRef refB, bool *tail_a) {
    const int lim = st.lim;
    LeanArgs a;
    a.g = pl.g; a.nd = lim; a.rdir = pl.flex; a.st = s->st; a.it = st.it; a.B = refB; a.R = c.refR; a.hist = s->hist;
    a.hist_cap = s->hist_cap; a.den = s->den;
    fill_dirs(a.d, s, 0, lim, LND);
    a.dir = st.dir; a.r = c.rcur; a.ar = s->ar; a.p_out = s->ps[0]; a.ap_out = s->aps[st.nxt]; a.n = pl.n; a.partsA = s->partsA;
    a.x = pl.x; a.lc = s->lc;
    PwTail pwa;
    if (pl.multi && lim <= ND && comm_pw_tail_begin(pl.comm, &pwa)) {
        pwa.pa = s->partsA; pwa.na = 4; pwa.pb = nullptr; pwa.nb = 0; pwa.out = s->dA; pwa.nblk = pl.g;
        a.pw = &pwa;
        *tail_a = true;
    }
    if (st.ic_next != 0) {
        // the next step is the solve's last and all it takes from this one are <r,Ap'>, <Ap',Ap'> (alpha_only_kernel: the caller — a
        // post-smoother's, a coarsest solve's — discards the residual): Ap' itself is never read, so it is not written
        if (g_skip_dead_ap.on() && c.global + 1 == pl.max_it && pl.skip_tail && pl.nested && s->discard_residual && !pl.multi)
            a.ap_out = nullptr;
        return launch_build_lean(a, 0);     // lim == nxt
    }
    if (lim <= ND) return launch_build_close(a);   // lim == restart: closes the cycle
    MGCR_TRY(launch_close_x(a));                   // ... in two kernels when restart > 8
    return launch_build_lean(a, 1);
}

// the classic build: p' and Ap' in chunks of ND stored directions
static int step_build_classic(GcrState *s, const SolvePlan &pl, const Step &st, RedRef refB, RedRef refR) {
    const int lim = st.lim, nchunk = (lim + ND - 1) / ND;
    for (int ch = 0; ch < nchunk; ch++) {
        BuildArgs a;
        a.g = pl.g;
        a.nd = lim - ch * ND < ND ? lim - ch * ND : ND;
        fill_dirs(a.d, s, ch * ND, a.nd, ND);
        a.first = ch == 0; a.last = ch == nchunk - 1; a.rdir = st.dir != s->r;
        // the step that closes a restart cycle streams every ps slot of the cycle: apply the deferred x updates there
        a.xupd = pl.defer && st.ic_next == 0;
        a.st = s->st; a.it = st.it; a.B = refB; a.book = a.last ? 1 : 0; a.R = refR; a.hist = s->hist; a.hist_cap = s->hist_cap;
        a.den = s->den; a.base = ch * ND; a.dir = st.dir; a.r = s->r; a.ar = s->ar; a.accp = s->accp; a.accap = s->accap;
        a.p_out = s->ps[st.nxt]; a.ap_out = s->aps[st.nxt]; a.n = pl.n; a.partsA = s->partsA; a.x = pl.x; a.alphas = s->alphas;
        MGCR_TRY(launch_build(a));
    }
    return MGCR_OK;
}

// apply + dots, then the build, with the multi-GPU reductions between and behind them
static int step_general(GcrState *s, const SolvePlan &pl, StepCursor &c, PhaseMarks &marks, const Step &st) {
    bool tail_rb = false, tail_a = false;
    MGCR_TRY(step_apply_dots(s, pl, c, st, &tail_rb));
    MGCR_TRY(marks.enter(2));
    RedRef refB = {s->partsB, pl.g, RED_MAX_BLOCKS};
    if (pl.multi) {  // one all-reduce for |r|^2 and all beta numerators of the step
        if (!tail_rb) MGCR_TRY(comm_fold_allreduce(pl.comm, s->partsR, 1, s->partsB, 2 * st.lim, s->dRB, pl.g));
        refB = {s->dRB + 1, 1, 1};
    }
    // (start1 makes every closing step a one-launch step: P0 is read from b only there)
    MGCR_CHECK(!(pl.start1 && st.ic_next == 0 && c.p0_live != s->ps[0]), MGCR_ERR_INVALID,
               "gcr: a cycle closed off the one-launch path after a one-launch start");
    if (pl.lean) MGCR_TRY(step_build_lean(s, pl, c, st, refB, &tail_a));
    else MGCR_TRY(step_build_classic(s, pl, st, refB, c.refR));
    if (pl.multi && !tail_a) MGCR_TRY(comm_fold_allreduce(pl.comm, s->partsA, 4, nullptr, 0, s->dA, pl.g));
    return MGCR_OK;
}

// one iteration, enqueued on the library stream; `it` = iteration number relative to DevState::base
static int gcr_step(GcrState *s, const SolvePlan &pl, StepCursor &c, PhaseMarks &marks, int it, bool last) {
    c.iter_count++;
    set_apply_skip(SkipRef{&s->st->stop_at, it});
    Step st;
    st.it = it; st.tail = last && pl.skip_tail;
    st.lim = s->storage < c.iter_count ? s->storage : c.iter_count;
    st.ic_next = c.iter_count % s->restart == 0 ? 0 : c.iter_count;
    st.nxt = st.ic_next % s->storage;
    MGCR_TRY(marks.enter(0));
    MGCR_TRY(ensure_slot(s, st.nxt));
    MGCR_TRY(pl.lean ? step_residual_lean(s, pl, c, st) : step_residual_classic(s, pl, c, st));
    if (!st.ended) {
        if (!s->r_after.empty() && c.global < (int)s->r_after.size()) s->r_after[(size_t)c.global] = pl.lean ? c.rcur : (const cplx *)s->r;
        if (st.tail) {
            MGCR_TRY(marks.enter(2));   // (the bookkeeping counts as the build phase)
            MGCR_TRY(step_finish(s, pl, c, st));
        } else {
            MGCR_TRY(marks.enter(1));
            if (step_is_one_launch(pl, st)) MGCR_TRY(step_one_launch(s, pl, c, marks, st));
            else MGCR_TRY(step_general(s, pl, c, marks, st));
        }
    }
    MGCR_TRY(marks.enter(3));
    c.iter_count = st.ic_next;
    c.cur = st.nxt;
    return MGCR_OK;
}

// hipGraph (opt-in, MGCR_GRAPH=1): in restart mode every cycle of R iterations is the same launch sequence with the
// same arguments (iteration numbers are base-relative, base lives on the device), so one cycle can be captured once
// and replayed.  Measured on MI355X: +11 % iterations/s on the 3072-row sample while an iteration was 4 launches;
// since it shrank to 3 (fused apply + dots) replay no longer pays at any size — eager launches run 1-4 % FASTER
// from 512 to 1.4 M rows (e.g. 64^3: 33.6 k against 32.3 k it/s), equal on the sample: the loop is bound by the
// GPU-side dependency between consecutive short kernels (~8 us each), not by the host's launch cost.  Hence off
// by default, and gated to <= 2^18 rows when on.
// The capture pass walks the cursor through one full cycle, which leaves it where it started: at the start of a cycle.
static int gcr_capture_cycle(GcrState *s, const SolvePlan &pl, StepCursor &c, PhaseMarks &marks) {
    const int R = s->restart;
    if (s->graph_exec && s->graph_x == pl.x && s->graph_R == R && s->graph_n == pl.n) return MGCR_OK;
    hipStream_t stream = ctx().stream;
    if (s->graph_exec) { hipGraphExecDestroy(s->graph_exec); s->graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    MGCR_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    int rc = MGCR_OK;
    for (int i = 1; i <= R && rc == MGCR_OK; i++) rc = gcr_step(s, pl, c, marks, i, false);
    if (rc == MGCR_OK) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, stream, s->st, R);
    }
    hipError_t e = hipStreamEndCapture(stream, &graph);
    if (rc != MGCR_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    MGCR_HIP(e);
    e = hipGraphInstantiate(&s->graph_exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    MGCR_HIP(e);
    s->graph_x = pl.x; s->graph_R = R; s->graph_n = pl.n;
    return MGCR_OK;
}

// the iterations: replayed cycle by cycle where a captured one exists, enqueued one by one otherwise; a top-level solve looks at
// the device-side stop predicate every check_every iterations
static int gcr_loop(GcrState *s, const SolvePlan &pl, StepCursor &c, PhaseMarks &marks) {
    Context &cx = ctx();
    const int R = s->restart, max_it = pl.max_it;
    const int check_every = s->p.check_every > 0 ? s->p.check_every : 10;
    int rel = 0;  // iterations enqueued eagerly since the last advance of DevState::base
    int last_check = 0;
    bool done = false;
    while (c.global < max_it && !done) {
        if (pl.use_graph && c.iter_count == 0 && rel == 0 && max_it - c.global >= R) {
            MGCR_HIP(hipGraphLaunch(s->graph_exec, cx.stream));
            c.global += R;
        } else {
            c.global++;
            rel++;
            MGCR_TRY(gcr_step(s, pl, c, marks, rel, c.global == max_it));
        }
        if (!pl.nested && (c.global / check_every != last_check || c.global == max_it)) {
            last_check = c.global / check_every;
            MGCR_HIP(hipMemcpyAsync(cx.h_mail, s->st, sizeof(DevState), hipMemcpyDeviceToHost, cx.stream));
            MGCR_HIP(hipStreamSynchronize(cx.stream));
            const DevState *hs = (const DevState *)cx.h_mail;
            if (hs->stop_at != INT_MAX) done = true;
        }
    }
    return MGCR_OK;
}

// x updates still pending (solve ended inside a restart cycle); ps[0..npend) hold their directions
static int gcr_flush_x(GcrState *s, const SolvePlan &pl) {
    DirPtrs d0;
    fill_dirs(d0, s, 0, s->storage, LND);
    d0.ps[0] = pl.p0;
    const cplx *coef = pl.lean ? (const cplx *)s->lc->cx : (const cplx *)s->alphas;
    if (pl.assign_x && s->keep_pending && pl.nested) {
        // the caller writes x = sum coef_j v_j itself, together with whatever else it has to add (V-cycle: + P x_c)
        for (int j = 0; j < LND; j++) s->pending.v[j] = d0.ps[j];
        s->pending.coef = coef;
        s->pending.st = s->st;
        s->has_pending = true;
        return MGCR_OK;
    }
    // (npend is not cleared afterwards: nothing reads it again before the next solve's reset_kernel zeroes it)
    KLAUNCH(flush_x_kernel, pl.g, s->st, coef, d0, pl.x, pl.n, pl.assign_x ? 1 : 0, pl.start1 ? pl.rhs : (const cplx *)nullptr);
    return MGCR_OK;
}

static int gcr_run_once(GcrState *s, const cplx *rhs, cplx *x, bool nested, double *hist, int hist_cap, int *n_iter, int *converged) {
    MGCR_CHECK(s->A, MGCR_ERR_INVALID, "GCR has no operator (call initialise / mgcr_gcr_set_operator first)");
    const int64_t n = s->A->dim;
    MGCR_TRY(gcr_prepare(s, n));
    const mgcr_gcr_param &p = s->p;
    const SkipRef outer = get_apply_skip();  // outer solver's predicate: if that solve is over, this one is a no-op too
    s->has_pending = false;
    s->defer_it = 0;
    s->partsN_of = nullptr;   // (set again by the start that leaves |b|^2 partials behind)
    const SolvePlan pl = gcr_plan(s, rhs, x, nested, s->x_from_zero);
    s->x_from_zero = false;

    if (pl.small) {
        if (pl.from_zero) MGCR_TRY(k_zero_apply(x, n));
        MGCR_TRY(ensure_slot(s, s->storage - 1));
        MGCR_TRY(gcr_small_run(s->A, p, s->storage, s->restart, rhs, x, s->r, s->ar, s->ps.data(), s->aps.data(), s->hist,
                               s->hist_cap, &s->st->stop_at));
        s->r_after.assign((size_t)pl.max_it + 1, (const cplx *)s->r);
        if (nested) return MGCR_OK;
        return gcr_finish(s, hist, hist_cap, n_iter, converged);
    }
    if (pl.resident) {
        if (!s->res_ring) MGCR_TRY(dalloc(&s->res_ring, (size_t)11 * n));   // the residual ring + P0 (freed with the other vectors)
        MGCR_TRY(gcr_resident_run(s->A, p, s->storage, s->restart, rhs, x, pl.from_zero, nested && s->discard_residual, s->st, s->hist,
                                  s->hist_cap, s->res_ring, outer));
        s->r_after.clear();
        if (nested) return MGCR_OK;
        MGCR_TRY(gcr_finish(s, hist, hist_cap, n_iter, converged));
        return resident_check(true);
    }

    hipLaunchKernelGGL(reset_kernel, dim3(1), dim3(1), 0, ctx().stream, s->st, outer.p, outer.it, p.tol * p.tol);
    MGCR_HIP(hipGetLastError());
    SkipGuard guard(SkipRef{&s->st->stop_at, 0});
    if (pl.from_zero && !pl.assign_x) MGCR_TRY(k_zero_apply(x, n));
    StepCursor cursor;
    PhaseMarks marks;
    marks.on = p.profile_spmv && !nested;
    MGCR_TRY(gcr_start(s, pl, cursor));
    if (pl.use_graph) {
        s->r_after.clear();   // replayed cycles do not pass through the host-side step counter
        MGCR_TRY(gcr_capture_cycle(s, pl, cursor, marks));
    }
    MGCR_TRY(gcr_loop(s, pl, cursor, marks));
    if (pl.defer) MGCR_TRY(gcr_flush_x(s, pl));
    if (nested) return MGCR_OK;
    MGCR_TRY(marks.read_out(pl));
    const int frc = gcr_finish(s, hist, hist_cap, n_iter, converged);
    if (pl.multi) MGCR_TRY(comm_check(pl.comm));   // a peer-write wait that timed out poisoned the scalars with NaN
    MGCR_TRY(resident_check(true));                // a one-launch step (gcr_stepbuild.hip) that was not co-resident gave up: gcr_run repeats the solve
    return frc;
}

// GCR::solve.  A top-level solve that took a one-launch path (gcr_resident.hip, gcr_stepbuild.hip: workgroups that wait for each
// other) and whose launch gave up — another process's kernels held CUs, so the grid was not co-resident; bounded polls, NaN
// results — is REPEATED here on the multi-kernel path, from the untouched right-hand side and the x the caller handed in: the
// caller gets the solve it asked for from its first call (mgcr_stat "one_launch_fallbacks" counts these).  The one-launch paths
// have switched themselves off by then (resident_check).  x on entry: zero when the caller says so (the Field was zeroed by
// mgcr_vec_zero and not written since: re-zeroed for the second run), otherwise a copy is kept whenever a one-launch path may run.
static int64_t g_fallbacks = 0;
int64_t gcr_fallback_count() { return g_fallbacks; }
int gcr_run(GcrState *s, const cplx *rhs, cplx *x, bool nested, double *hist, int hist_cap, int *n_iter, int *converged, bool x_known_zero) {
    if (nested) return gcr_run_once(s, rhs, x, true, hist, hist_cap, n_iter, converged);
    MGCR_CHECK(s->A, MGCR_ERR_INVALID, "GCR has no operator (call initialise / mgcr_gcr_set_operator first)");
    const int64_t n = s->A->dim;
    // Which solves can meet a one-launch path at all?  The solve itself up to 2^21 rows (the paths' own conditions are narrower —
    // operator kind, storage, restart length — but none of them takes more); at any size when a preconditioner is attached, whose
    // nested solves (an MG cycle's coarsest level) may take one.  A copy too many costs one pass over x.
    const bool risky = one_launch_paths_enabled() && comm_live_count() == 0 &&
                       (n <= ((int64_t)1 << 21) || s->p.left_precond || s->p.right_precond);
    bool have_copy = false;
    if (risky && !x_known_zero) {
        if (s->xbak_n != n) {
            hipStreamSynchronize(ctx().stream);
            hipFree(s->xbak); s->xbak = nullptr; s->xbak_n = 0;
            MGCR_TRY(dalloc(&s->xbak, (size_t)n));
            s->xbak_n = n;
        }
        MGCR_TRY(k_copy(s->xbak, x, n));
        have_copy = true;
    }
    int rc = gcr_run_once(s, rhs, x, false, hist, hist_cap, n_iter, converged);
    if (rc != MGCR_INT_GAVE_UP) return rc;
    if (!have_copy && !x_known_zero) {   // (cannot happen: nothing that waits on other workgroups ran) — report like a host synchronisation point would
        set_error("one-launch solver kernel gave up and no copy of x was kept");
        return MGCR_ERR_HIP;
    }
    if (have_copy) MGCR_TRY(k_copy(x, s->xbak, n));
    else MGCR_TRY(k_zero(x, n));
    g_fallbacks++;
    rc = gcr_run_once(s, rhs, x, false, hist, hist_cap, n_iter, converged);
    return rc == MGCR_INT_GAVE_UP ? MGCR_ERR_HIP : rc;
}

void gcr_set_discard_residual(GcrState *s, bool on) { s->discard_residual = on; }
void gcr_set_bnorm_source(GcrState *s, GcrState *src) { s->bnorm_src = src; }
void gcr_set_keep_pending(GcrState *s, bool on) { s->keep_pending = on; }
// x = sum coef_j v_j for a caller that took the pending update and then needs x after all
int gcr_flush_pending(const PendingX &pd, cplx *x, int64_t n) {
    DirPtrs d0;
    for (int j = 0; j < LND; j++) { d0.ps[j] = pd.v[j]; d0.aps[j] = pd.v[j]; d0.slot[j] = j; }
    hipLaunchKernelGGL(flush_x_kernel, dim3(red_grid(n)), dim3(RED_THREADS), 0, ctx().stream, const_cast<DevState *>(pd.st), pd.coef, d0, x, n, 1,
                       (const cplx *)nullptr);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}
// did the solve that just ran leave x unwritten (see keep_pending)?  Then *out says what x is.
bool gcr_take_pending(GcrState *s, PendingX *out) {
    if (!s->has_pending) return false;
    *out = s->pending;
    s->has_pending = false;
    return true;
}

// the residual of the solve that just ran on `s`, selected on the device by the number of steps it took
bool gcr_last_residual(GcrState *s, ResidualSel *out) {
    if (s->r_after.size() < 2 || s->r_after.size() > (size_t)LND + 1) return false;
    for (size_t k = 1; k < s->r_after.size(); k++)
        if (!s->r_after[k]) return false;
    for (int k = 0; k <= LND; k++) out->r[k] = s->r_after[(size_t)k < s->r_after.size() ? (size_t)k : s->r_after.size() - 1];
    out->r[0] = s->r_after[1];
    out->st = s->st;
    out->r_prev = s->defer_it ? s->defer_r_prev : nullptr;
    out->ap = s->defer_ap;
    out->alpha = s->defer_alpha;
    out->last_it = s->defer_it;
    return true;
}
void gcr_set_defer_residual(GcrState *s, bool on) { s->defer_residual = on; }

// nested solve from x0 = 0 into an x whose content does not matter (smoothers, coarsest solve, GCR as a preconditioner)
int gcr_run_from_zero(GcrState *s, const cplx *rhs, cplx *x) {
    s->x_from_zero = true;
    return gcr_run(s, rhs, x, true, nullptr, 0, nullptr, nullptr);
}

// x = init_rand(2) in the reference (src/GCR.h:63-68); here the caller-provided x0 or zero
int gcr_apply_as_operator(GcrState *s, const cplx *f, cplx *y) {
    MGCR_CHECK(s->A, MGCR_ERR_INVALID, "GCR has no operator (call initialise / mgcr_gcr_set_operator first)");
    const int64_t n = s->A->dim;
    if (s->x0_mode == 0 && s->x0) MGCR_TRY(k_copy_apply(y, s->x0, n));
    else return gcr_run_from_zero(s, f, y);
    return gcr_run(s, f, y, true, nullptr, 0, nullptr, nullptr);
}

}  // namespace mgcr
