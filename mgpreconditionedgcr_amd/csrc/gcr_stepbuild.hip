// A lean GCR step as ONE launch (src/GCR.h:230-287), for systems whose A r fits the chip's LDS: at most 4096 rows per
// workgroup of 1024 threads, two workgroups per CU — 2 097 152 rows on MI355X, i.e. up to Poisson 128^3, the metric's
// configuration.
//
// gcr_fused.hip's step_apply_kernel writes Ar (V), its partial sums of <Ar, Ap_j> go to memory, and gcr.hip's
// build_lean_kernel — behind a kernel boundary, because beta needs the sums over ALL workgroups — reads Ar back (V);
// xr_update_kernel, behind another boundary because alpha needs <r,Ap'> and <Ap',Ap'>, reads r and the new Ap' back.
// Here the kernel bodies run in one launch with exchange_dev.h's fence-free exchange (~3 us) where the boundaries were:
//   apply + dots | exchange | direction build (CLOSE: the cycle-closing form, gcr.hip build_close_kernel: x update and the
//   next cycle's first direction in a pass of their own) | exchange | XR: the NEXT step's residual update.
// A thread keeps the Ar of its 4 rows in LDS (64 KB per workgroup, thread-private slots) and overwrites it with the new
// Ap' for the update: Ar is neither written to nor read from memory, Ap' is not read back — per in-cycle step
// B_matrix + 16 ncol + (2 lim + 4) V instead of B_matrix + 16 ncol + (2 lim + 7) V, two kernel boundaries and two folds
// less.  The first trip's streams of the build and the update's first r are requested before an exchange is polled.
// Everything else is the kernels' code: the same rows per thread (RowMap), the same per-thread accumulation order, the
// same fold tree — the same bits (tests/test_gpu_stepbuild.py compares with the three-kernel path bit for bit).
// The scalar stage between "the sums have arrived" and "stream the rows" (step bookkeeping, the coefficient table's row, the
// closing coefficients) IS the three-kernel path's: gcr_dev.h; the exchange scaffolding is exchange_dev.h's.
// Up to 3 stored directions (the closing step with XR at 3 excepted) step_keep_kernel runs the step, reading r once; at 4 with XR
// and at the close at 5 step_keep_wide_kernel does: the same body (gcr_stepbuild_keep_body.h) under another compile-time policy
// (SbKeepPolicy).  Everywhere else, and as the reference side of tests/test_gpu_stepbuild_keep_all.py and
// tests/test_gpu_stepbuild_keep_wide.py, step_build_kernel.
// The body is a text included into the two kernel templates, not a __device__ function template: called through a forceinline
// function (by value or by reference, its LDS declared inside or handed in) step_keep_kernel<3, true, false, false> needs 8 B of
// scratch per lane and step_keep_kernel<2, true, true, false> 64 instead of 61 VGPRs; included, the old name's code is what it was.
// Neither reads from memory what it holds: the keep body's build takes its first Ap_0 rows from the registers of the pass-1
// dots (sb_kept_rows: per form as many as fit, step_keep_wide_kernel included), and the closing step_build_kernel at 4 and 5 directions loads a row's r once for the close pass and the
// build, which are one loop there, the thread's last close row behind the exchange-2 publish (sb_close_merged;
// tests/test_gpu_stepbuild_reuse.py: the same bits, tests/test_stepbuild_reuse_regs.py: the same registers class).
// The keep body's scalar stage behind exchange 1 reads nothing from memory either: its operands are fetched behind the apply and
// parked in LDS, the |r|^2 fold and the stop decision are made ahead of the poll (tests/test_gpu_stepbuild_scalar_stage.py,
// tests/test_stepbuild_scalar_stage_regs.py).
// The keep forms for real coefficients do not load a row's own r either: it IS the diagonal slot's gather (sb_apply_form; a trip of
// their apply is 7 loads and one round trip where it was 8 and two; 34.8 against 36.7 us at 1 direction, +1.5 % on the headline).
// Taking r[i - 1] and r[i + 1] from the neighbouring lanes on top of that (6 loads per trip) gives the same bits and was measured
// slower: not built.  tests/test_gpu_stepbuild_apply_lanes.py, tests/test_stepbuild_apply_lanes_regs.py, DESIGN section 8.
//
// Needs all workgroups co-resident (they wait for each other): 64 VGPRs and <= 80 KB of LDS each, at most 2 x #CU
// workgroups, no other process on the device (no live communicator).  Up to 5 stored directions (beyond that the
// kernels need 128 registers: one workgroup per CU).  Bounded polls as in gcr_resident.hip: a missing workgroup makes the
// others leave with NaN results, the solve returns an error and the one-launch paths switch themselves off.
// The host (gcr.hip gcr_step) knows which launch already performed the next update (StepCursor::xr_prefetched); a solve that stops
// on the device turns the whole launch, or its update part, into a no-op like any other kernel of the solve.
#include <climits>
#include <cstdlib>
#include <type_traits>

#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "spmv_dev.h"
#include "exchange_dev.h"
#include "gcr_stepbuild_dev.h"   // the argument block and the helpers shared with gcr_steppair.hip

namespace mgcr {

constexpr int SB_KEEP_TB = 2;      // step_keep_kernel: trips whose streams are in registers at a time
// The keep body: rows of Ap_0 (the thread's first trips) that stay in registers from the pass-1 dots to the build.  Per form, the
// most with which it compiles to 0 scratch and 8 waves per SIMD, the scalar stage's early loads in place (one row more needs 8 to
// 48 B per lane everywhere; tests/test_stepbuild_scalar_stage_regs.py pins the table and the resources).  At 1 direction with
// the next residual update, 3: tests/test_stepbuild_apply_lanes_regs.py pins that form's loads; 4 has not been tried in the others.
// The forms for complex coefficients keep what they had (2, none in step_keep_wide_kernel): three of them need scratch for one more.
// -DMGCR_SB_KEEP_MORE=0 builds those counts for every form, for a measurement.
#ifndef MGCR_SB_KEEP_MORE
#define MGCR_SB_KEEP_MORE 1
#endif
template <bool WIDE, int NDT, bool XR, bool CLOSE, bool REALC> constexpr int sb_kept_rows() {
    if (NDT == 1) return 3;
    if (!REALC || !MGCR_SB_KEEP_MORE) return WIDE ? 0 : 2;
    if (!WIDE) return !XR && CLOSE ? 4 : 3;   // 2 and 3 directions
    if (NDT == 4) return CLOSE ? 4 : 1;
    return XR ? 2 : 3;                        // the close at 5
}
// The rows of Ap_0 that are NOT kept are the last stream pass 1 loads and the first the build loads (<= 1 MB per XCD and row):
// loaded temporally in pass 1, the build's re-read can hit the XCD's L2.  Built in the three forms of the headline whose own
// trace showed it faster; at 2 and 3 directions the mixed loads cost 20-24 B of scratch and time, the other
// forms were not measured.  -DMGCR_SB_TEMPORAL_TAIL=1 / 0 builds it in every form / in none, for a measurement.
#ifndef MGCR_SB_TEMPORAL_TAIL
#define MGCR_SB_TEMPORAL_TAIL -1
#endif
template <bool WIDE, int NDT, bool XR, bool CLOSE, bool REALC> constexpr bool sb_temporal_tail() {
    if (MGCR_SB_TEMPORAL_TAIL >= 0) return MGCR_SB_TEMPORAL_TAIL != 0;
    return REALC && XR && (WIDE ? (NDT == 4 && !CLOSE) || (NDT == 5 && CLOSE) : NDT == 1 && !CLOSE);
}
// The compile-time policy of the keep body (gcr_stepbuild_keep_body.h): trips per batch of the build and the close pass, rows of Ap_0 kept across exchange 1, and
// whether the trips' byte offsets are formed on the fly (trip 0's + t x the row step) instead of held, one register per trip
// ... how the apply gets the thread's own r and its two neighbours in the row (sb_apply_form), and whether pass 1 loads the rows
// of Ap_0 it does not keep temporally (sb_temporal_tail)
template <int TB_, int KT_, bool OTF_, int APPLY_, bool TAIL_> struct SbKeepPolicy {
    static constexpr int TB = TB_, KT = KT_;
    static constexpr bool OTF = OTF_, TAIL = TAIL_;   // TAIL: sb_temporal_tail
    static constexpr bool OWN = APPLY_ >= 1, LANES = APPLY_ >= 2;
};
// The apply of a keep form: 0 the seven gathers and a load of the row's own r behind them; 1 the own r IS the diagonal slot's
// gather (one load and one dependent round trip less per trip); 2 r[i - 1] and r[i + 1] come from the neighbouring lanes as well
// (spmv_dev.h sten_row_product_own_t).  1 and 2 need sten_lane_middle(A): the host checks it (sb_kernel).
// Built: 1 in every form for real coefficients.  2 fits them all (0 scratch, 60..64 VGPRs) and gives the same bits, but was
// measured slower than 1 in each of the headline's five kernels; -DMGCR_SB_APPLY=2 / 0 builds it / the old apply
// for such a measurement.  The forms for complex coefficients keep 0: with 1 or 2 every one of them needs 12 to 20 B of scratch
// (their scalar registers already spill into vector-register lanes).
#ifndef MGCR_SB_APPLY
#define MGCR_SB_APPLY 1
#endif
template <bool WIDE, int NDT, bool XR, bool CLOSE, bool REALC> constexpr int sb_apply_form() { return REALC ? MGCR_SB_APPLY : 0; }
// step_build_kernel<CLOSE>: the forms whose close pass and build are one loop over the rows — those it costs no scratch (at 3
// directions the build's prefetched first row lives longer: 28 B; at 5 without the next residual update, a solve's last step: 12 B)
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_close_merged() { return CLOSE && (NDT == 4 || (NDT == 5 && XR)); }

// REALC: the instantiation for real stencil coefficients (no per-slot real / complex decision, 14 scalar registers less — the
// kernels' scalar registers spill into vector-register lanes, which a wave then reads back one v_readlane at a time)
template <int MODE, int WT, int NDT, bool XR, bool CLOSE, bool REALC = false>
__global__ void __launch_bounds__(RED_THREADS, 8) step_build_kernel(StepBuildArgs a) {
    __shared__ double lds[(2 * NDT > 4 ? 2 * NDT : 4) * 17];
    __shared__ double lds_pw[2 * SB_MAX_ND * 17], lds_ws[2 * SB_MAX_ND * RES_GRP];
    __shared__ int gave_up;
    __shared__ cplx sbeta[NDT], scp[NDT];
    extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];   // Ar of this workgroup's rows: [trip][thread]
    if (a.st->stop_at < a.st->base + a.it) return;
    const int lb = logical_workgroup(a.rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= a.nlogical) return;
    cplx *arL = reinterpret_cast<cplx *>(sb_smem);
    ResSync sy;
    res_sync_init(sy, a.slots, a.gen0, a.nlogical, lb, a.abort_dev, a.spin_limit, lds_pw, lds_ws, &gave_up);
    if (a.test_stall && lb == a.test_stall - 1) return;   // (tests) the others must notice, give up and say so
    int64_t i0, end, stride;
    row_range(a.rm, lb, a.nlogical, a.n, &i0, &end, &stride);
    // ---- apply + dot products (gcr_fused.hip step_apply_kernel) ----
    {
        double v[2 * NDT];
#pragma unroll
        for (int j = 0; j < 2 * NDT; j++) v[j] = 0.;
        int trip = 0;
        for (int64_t i = i0; i < end; i += stride, trip++) {
            const PatLds pl{nullptr, nullptr, nullptr};
            cplx sum;
            if constexpr (REALC) sum = sten_row_product_t<WT, false, 1>(a.m, i, [&](int32_t j) -> cplx { return a.x[j]; });
            else sum = fused_row_product<MODE, WT>(a.m, i, 0, pl, [&](int32_t j) -> cplx { return a.x[j]; });
            const cplx yi = a.m.shift ? csub(a.x[i], cmul(a.m.k, sum)) : sum;
            arL[trip * RED_THREADS + (int)threadIdx.x] = yi;
            __builtin_amdgcn_sched_barrier(0);
            cplx b[NDT];
#pragma unroll
            for (int j = 0; j < NDT; j++) b[j] = ld_stream<true>(a.aps[j] + i);
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx t = cconj_mul(yi, b[j]);
                v[2 * j] += t.x;
                v[2 * j + 1] += t.y;
            }
        }
        // ---- the sums over all workgroups (exchange_dev.h), in place of the partial slab + fold_partials ----
        const double mine = block_sum_owner<2 * NDT>(v, lds);
        if ((int)threadIdx.x < 2 * NDT) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((1 * RES_NV + (int)threadIdx.x) * RES_BLK + lb) * 16, 0, RES_SC1);
        }
    }
    // the first trip's streams of the build are requested BEFORE the exchange is waited for (they do not depend on beta): one
    // memory round trip of the launch hides behind the polls
    // (up to 3 stored directions: with more the kernel does not keep them next to everything else in 64 registers)
    constexpr bool PRE = NDT <= 3;
    cplx pre[NDT];
#pragma unroll
    for (int j = 0; j < NDT; j++) pre[j] = make_double2(0., 0.);
    if (PRE && i0 < end) {
#pragma unroll
        for (int j = 0; j < NDT; j++) pre[j] = ld_stream<NTS>((CLOSE ? a.ps[j] : a.aps[j]) + i0);
    }
    const bool ok = res_collect<2 * NDT>(sy, 1);
    if (!ok) {   // somebody is missing: leave, with results nobody can mistake for numbers
        res_abort(a.abort_dev, a.abort_host);
        for (int64_t i = i0; i < end; i += stride) a.ap_out[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
        if ((int)threadIdx.x < 4) a.partsA[threadIdx.x * RED_MAX_BLOCKS + lb] = __builtin_nan("");
        return;
    }
    // ---- direction build (gcr.hip build_lean_kernel, not closing) ----
    bool ends_here = false;   // XR: did this step end the solve?  Every workgroup folds |r|^2 itself: same bits, same answer
    if (XR || lb == 0) {
        double rr[1];
        fold_partials<1>(a.partsR, a.nblkR, a.strideR, rr, lds);
        if (lb == 0 && threadIdx.x == 0) {
            close_step(a.st, a.it, rr[0], a.hist, a.hist_cap, CLOSE);
            if (CLOSE) a.st->closed = 1;   // (P0' is written below, by every workgroup that reaches the close pass)
        }
        ends_here = gcr_solve_ends(rr[0], a.st->bnorm2, a.st->tol2);
    }
    if ((int)threadIdx.x < NDT) sbeta[threadIdx.x] = cdiv(make_double2(res_total(sy, 2 * threadIdx.x), res_total(sy, 2 * threadIdx.x + 1)), a.den[threadIdx.x]);
    __syncthreads();
    if constexpr (CLOSE) {   // gcr.hip build_close_kernel: cp_m = sum_{j >= m} beta_j T_jm (cp_0 = sum_j beta_j t_j), in every workgroup
        if ((int)threadIdx.x < NDT) scp[threadIdx.x] = lean_close_coef(a.lc, sbeta, NDT, (int)threadIdx.x);
        __syncthreads();
    }
    if (!CLOSE && lb == 0 && (int)threadIdx.x <= NDT) lean_table_row<NDT>(a.lc, sbeta, (int)threadIdx.x);   // row k = NDT of the table
    cplx beta[NDT];
#pragma unroll
    for (int j = 0; j < NDT; j++) beta[j] = to_sgpr(sbeta[j]);
    double v[4] = {0., 0., 0., 0.};
    int trip = 0;
    // CLOSE with 4 or 5 directions: ONE loop over the rows — r of a row is loaded once for its close row and its build row — and
    // the thread's last close row waits until the exchange-2 partials are on their way (sb_close_merged)
    constexpr bool MERGED = sb_close_merged<NDT, XR, CLOSE>();
    cplx mcp[MERGED ? NDT : 1], mcx[MERGED ? NDT : 1];
    if constexpr (MERGED) {
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            mcp[j] = to_sgpr(scp[j]);
            mcx[j] = to_sgpr(a.lc->cx[j]);   // (before this workgroup publishes: workgroup 0 rewrites lc->cx behind poll 2)
        }
    }
    // x += sum_j cx_j p_j;  P0' = r - sum_j cp_j p_j for one row, as in the close pass below: p_out = ps[0] is read before it is
    // written, and xr_out = ps[1] is read here before XR writes it (every close row precedes poll 2)
    auto close_row = [&](int64_t i, cplx dv) {
        cplx pj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) pj[j] = ld_stream<NTS>(a.ps[j] + i);
        cplx xv = a.xvec[i];
#pragma unroll
        for (int j = 0; j < NDT; j++) xv = cadd(xv, cmul(mcx[MERGED ? j : 0], pj[j]));
        a.xvec[i] = xv;
        cplx pc = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++) pc = csub(pc, cmul(mcp[MERGED ? j : 0], pj[j]));
        st_stream<NTS>(a.p_out + i, cadd(dv, pc));
    };
    if constexpr (CLOSE && !MERGED) {
        // x += sum_j cx_j p_j;  P0' = dir - sum_j cp_j p_j  (p_0 = P0, p_m = D_m): a pass of its own over the p streams, so that they
        // and the Ap streams below are never in registers together (64 VGPRs: two workgroups per CU)
        cplx cp[NDT], cx[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            cp[j] = to_sgpr(scp[j]);
            cx[j] = to_sgpr(a.lc->cx[j]);
        }
        for (int64_t i = i0; i < end; i += stride) {
            cplx pj[NDT];
#pragma unroll
            for (int j = 0; j < NDT; j++) pj[j] = (PRE && i == i0) ? pre[j] : ld_stream<NTS>(a.ps[j] + i);
            const cplx dv = a.x[i];
            cplx xv = a.xvec[i];
#pragma unroll
            for (int j = 0; j < NDT; j++) xv = cadd(xv, cmul(cx[j], pj[j]));
            a.xvec[i] = xv;
            cplx pc = make_double2(0., 0.);
#pragma unroll
            for (int j = 0; j < NDT; j++) pc = csub(pc, cmul(cp[j], pj[j]));
            st_stream<NTS>(a.p_out + i, cadd(dv, pc));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // (kept as a lambda that returns the row's r: written as the loop's body, the same statements change the registers of thirty
    // instantiations — profiles/scalar_stage_refactor_resource_usage.md)
    auto build_row = [&](int64_t i, int trip, cplx r_have) -> cplx {   // r_have: the row's r, where the caller holds it (MERGED)
        cplx aj[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) aj[j] = (PRE && !CLOSE && i == i0) ? pre[j] : ld_stream<NTS>(a.aps[j] + i);
        const cplx av = arL[trip * RED_THREADS + (int)threadIdx.x], rv = MERGED ? r_have : a.x[i];
        cplx ac = make_double2(0., 0.);
#pragma unroll
        for (int j = 0; j < NDT; j++) ac = csub(ac, cmul(beta[j], aj[j]));
        const cplx an = cadd(av, ac);
        a.ap_out[i] = an;
        if (XR) arL[trip * RED_THREADS + (int)threadIdx.x] = an;   // (A r is not needed any more; the update below wants Ap')
        cplx t = cconj_mul(rv, an);
        v[0] += t.x; v[1] += t.y;
        cplx u = cconj_mul(an, an);
        v[2] += u.x; v[3] += u.y;
        return rv;
    };
    if constexpr (MERGED) {
        for (int64_t i = i0; i < end; i += stride, trip++) {
            const cplx rv = a.x[i];
            if (!XR || i + stride < end) close_row(i, rv);   // (XR: the thread's last row waits for the publish below)
            __builtin_amdgcn_sched_barrier(0);   // (the p streams and the Ap streams are never in registers together)
            (void)build_row(i, trip, rv);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int64_t i = i0; i < end; i += stride, trip++) (void)build_row(i, trip, make_double2(0., 0.));
    }
    const double mine = block_sum_owner<4>(v, lds);
    if (threadIdx.x < 4) a.partsA[threadIdx.x * RED_MAX_BLOCKS + lb] = mine;
    // MERGED with XR: the thread's last close row (its r loaded again: kept across the block sum it spills) behind the publish
    auto close_last = [&]() {
        if (trip > 0) {
            const int64_t il = i0 + (int64_t)(trip - 1) * stride;
            close_row(il, a.x[il]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (XR) {
        // ---- the next step's residual update (gcr.hip xr_update_kernel<true, true>): alpha needs <r,Ap'>, <Ap',Ap'> over ALL
        // workgroups — a second exchange instead of a kernel boundary; r and Ap' of the thread's rows are on the chip ----
        if ((int)threadIdx.x < 4) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((2 * RES_NV + (int)threadIdx.x) * RES_BLK + lb) * 16, 0, RES_SC1);
        }
        if constexpr (MERGED) close_last();   // (streams while the exchange-2 partials travel)
        const cplx xr0 = i0 < end ? a.x[i0] : make_double2(0., 0.);   // (requested before the polls, like `pre` above)
        if (!res_collect<4>(sy, 2)) {
            res_abort(a.abort_dev, a.abort_host);
            for (int64_t i = i0; i < end; i += stride) a.xr_out[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
            if (threadIdx.x == 0) a.partsR_out[lb] = __builtin_nan("");
            return;
        }
        if (ends_here) return;   // the step converged: the next one's kernels are no-ops (gcr_dev.h DevState::stop_at)
        const cplx alpha = sb_xr_alpha(sy, a.st, a.lc, a.xr_den_slot, a.xr_slot, lb);
        double vr[1] = {0.};
        trip = 0;
        for (int64_t i = i0; i < end; i += stride, trip++) {
            const cplx rn = csub(i == i0 ? xr0 : a.x[i], cmul(alpha, arL[trip * RED_THREADS + (int)threadIdx.x]));
            a.xr_out[i] = rn;
            vr[0] += rn.x * rn.x + rn.y * rn.y;
        }
        const double tot = block_sum_owner<1>(vr, lds);
        if (threadIdx.x == 0) a.partsR_out[lb] = tot;
    }
}

// KEEP-ALL (the body is gcr_stepbuild_keep_body.h): step_build_kernel's step (in-cycle / closing, with / without XR) with r read
// ONCE per launch: the thread's residual rows ARE the apply's diagonal gathers (sb_apply_form; the forms for complex coefficients
// load them again behind the gathers: the same lines, a cache hit) and stay in registers (SB_MAX_TRIPS x
// 16 B) for the shift epilogue, the build's <r,Ap'>, the close pass's P0' and XR; no later pass loads a.x.
// Register use: the pass-1 dots walk one direction (all trips) at a time, the last direction first, and hand its two sums to the
// wave trees as soon as they are final (sb_wave_pair_to_lds: the bits of block_sum_owner<2 NDT>, whatever the order of the
// directions); the first sb_kept_rows rows of Ap_0, which the dots load last, stay in registers across exchange 1 for the build
// (no stream is requested ahead of that exchange's polls any more); the build and the close pass walk SB_KEEP_TB trips at a
// time, one direction after the other; every stream is addressed as scalar base + one 32-bit offset per trip.  Every element sees
// the same operations in the same order as in step_build_kernel (ac -= beta_j Ap_j in j order, each per-thread accumulator adds
// the rows in trip order): the same bits.  Only the forms that fit 64 VGPRs without scratch are launched (sb_keep_fits).
// With 4 and 5 directions that policy spills (48 B at 4); step_keep_wide_kernel's does not: the build and the close pass walk ONE
// trip at a time, 1 to 4 rows of Ap_0 are kept across exchange 1 (sb_kept_rows; the build loads the others: a pass-1 line it
// re-reads directly behind pass 1, from the XCD's L2 where sb_temporal_tail says so), and at 5 with XR only trip 0's offset is held, the others formed as off[0] + t x (row step in bytes, a scalar register)
// where they are used — written as that one sum: added to the scalar base first, the form costs 20 B.  The policies are
// `if constexpr` on POL only: forming the offsets on the fly in step_keep_kernel<3, true, false, *> costs it 20 B.
// CLOSE runs build | publish exchange 2 | close pass | poll 2 | XR: the build's Ap_j re-reads follow pass 1 closely, and the close
// pass (x update and P0', which need only beta and cp) runs while the exchange-2 partials travel.  xr_out = ps[1] (read by the
// close pass) and p_out = ps[0]: a thread reads an element of them before it writes it, and no other thread touches it; lc->cx,
// which workgroup 0 updates behind poll 2, is read before this workgroup publishes.
template <int NDT, bool XR, bool CLOSE, bool REALC>
__global__ void __launch_bounds__(RED_THREADS, 8) step_keep_kernel(StepBuildArgs a) {
    using POL = SbKeepPolicy<SB_KEEP_TB, sb_kept_rows<false, NDT, XR, CLOSE, REALC>(), false, sb_apply_form<false, NDT, XR, CLOSE, REALC>(),
                             sb_temporal_tail<false, NDT, XR, CLOSE, REALC>()>;
#include "gcr_stepbuild_keep_body.h"
}
// 4 stored directions with XR, 5 at the close (sb_keep_wide_fits): one trip at a time, at 5 with XR the offsets on the fly
template <int NDT, bool XR, bool CLOSE, bool REALC>
__global__ void __launch_bounds__(RED_THREADS, 8) step_keep_wide_kernel(StepBuildArgs a) {
    using POL = SbKeepPolicy<1, sb_kept_rows<true, NDT, XR, CLOSE, REALC>(), NDT == 5 && XR, sb_apply_form<true, NDT, XR, CLOSE, REALC>(),
                             sb_temporal_tail<true, NDT, XR, CLOSE, REALC>()>;
#include "gcr_stepbuild_keep_body.h"
}

// The start of a solve from x0 = 0 as ONE launch (r0 = P0 = b, no preconditioner): what gcr.hip ran as copy2_kernel (r = P0 = b),
// gcr_fused.hip init_apply_kernel (Ap0 = A b and the partials of <b,Ap0>, <Ap0,Ap0>, |b|^2), init_kernel (|b|^2, hist[0]) and
// step 1's xr_update_kernel<true, true> (alpha, r1 = b - alpha Ap0 into the residual ring, its |r1|^2 partials):
//   apply + sums | exchange | bookkeeping (logical workgroup 0) | alpha, r1.
// Ap0 stays in LDS for the update (and is written once, as aps[0]); b is read again by the update, its first row requested before
// the poll (kept in registers instead, the kernel needs scratch); r and P0 are never copied — cycle 1 reads b where it read them.  The same rows per thread (RowMap), the same per-thread accumulation order,
// the same fold tree as those kernels: the same bits.  |b|^2 and |r0|^2 are one sum here, as they were two folds of the same
// partials there.  Needs what step_build_kernel needs (co-residency, bounded polls, give-up with NaN results).
struct StartArgs {
    RowMat m;
    const cplx *b;
    cplx *ap0;
    int64_t n;
    int nlogical;
    RowMap rm;
    DevState *st;
    double *hist;
    LeanCoef *lc;
    cplx *den0;
    cplx *r_out;             // r1 (the ring slot of step 1)
    double *partsR_out;
    v4i *slots;
    unsigned gen0;
    unsigned *abort_dev;
    int *abort_host;
    int spin_limit;
    int test_stall;
};

template <bool REALC>
__global__ void __launch_bounds__(RED_THREADS, 8) start_build_kernel(StartArgs a) {
    __shared__ double lds[6 * 17];
    __shared__ double lds_pw[2 * SB_MAX_ND * 17], lds_ws[2 * SB_MAX_ND * RES_GRP];
    __shared__ int gave_up;
    extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];   // Ap0 of this workgroup's rows: [trip][thread]
    if (a.st->stop_at < 0) return;   // (an outer solve that is over: reset_kernel)
    const int lb = logical_workgroup(a.rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= a.nlogical) return;
    cplx *apL = reinterpret_cast<cplx *>(sb_smem);
    ResSync sy;
    res_sync_init(sy, a.slots, a.gen0, a.nlogical, lb, a.abort_dev, a.spin_limit, lds_pw, lds_ws, &gave_up);
    if (a.test_stall && lb == a.test_stall - 1) return;
    int64_t i0, end, stride;
    row_range(a.rm, lb, a.nlogical, a.n, &i0, &end, &stride);
    // ---- Ap0 = A b and the sums (init_apply_kernel: v[4] = |r0|^2, v[5] = |b|^2 stays 0 as there, b IS r0) ----
    {
        double v[6] = {0., 0., 0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < SB_MAX_TRIPS; t++) {
            const int64_t i = i0 + (int64_t)t * stride;
            if (i < end) {
                const PatLds pl{nullptr, nullptr, nullptr};
                cplx sum;
                if constexpr (REALC) sum = sten_row_product_t<7, false, 1>(a.m, i, [&](int32_t j) -> cplx { return a.b[j]; });
                else sum = fused_row_product<3, 7>(a.m, i, 0, pl, [&](int32_t j) -> cplx { return a.b[j]; });
                const cplx rv = a.b[i];
                const cplx yi = a.m.shift ? csub(rv, cmul(a.m.k, sum)) : sum;
                a.ap0[i] = yi;
                apL[t * RED_THREADS + (int)threadIdx.x] = yi;
                v[4] += rv.x * rv.x + rv.y * rv.y;
                const cplx tt = cconj_mul(rv, yi);
                v[0] += tt.x; v[1] += tt.y;
                const cplx u = cconj_mul(yi, yi);
                v[2] += u.x; v[3] += u.y;
            }
            __builtin_amdgcn_sched_barrier(0);   // (one trip's gathers in registers at a time)
        }
        const double mine = block_sum_owner<6>(v, lds);
        if ((int)threadIdx.x < 5) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((1 * RES_NV + (int)threadIdx.x) * RES_BLK + lb) * 16, 0, RES_SC1);
        }
    }
    const cplx b0 = i0 < end ? a.b[i0] : make_double2(0., 0.);   // (requested before the polls)
    if (!res_collect<5>(sy, 1)) {
        res_abort(a.abort_dev, a.abort_host);
        for (int64_t i = i0; i < end; i += stride) a.r_out[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
        if (threadIdx.x == 0) a.partsR_out[lb] = __builtin_nan("");
        return;
    }
    // ---- init_kernel's bookkeeping, then xr_update_kernel<true, true> of step 1 (slot 0) ----
    if (lb == 0 && threadIdx.x == 0) {
        const double nb = res_total(sy, 4);
        a.st->bnorm2 = nb;
        a.st->rr = nb;
        a.hist[0] = sqrt(nb) / sqrt(nb);
    }
    const cplx alpha = sb_xr_alpha(sy, a.st, a.lc, a.den0, 0, lb);
    double vr[1] = {0.};
#pragma unroll
    for (int t = 0; t < SB_MAX_TRIPS; t++) {
        const int64_t i = i0 + (int64_t)t * stride;
        if (i < end) {
            const cplx rn = csub(t == 0 ? b0 : a.b[i], cmul(alpha, apL[t * RED_THREADS + (int)threadIdx.x]));
            a.r_out[i] = rn;
            vr[0] += rn.x * rn.x + rn.y * rn.y;
        }
    }
    const double tot = block_sum_owner<1>(vr, lds);
    if (threadIdx.x == 0) a.partsR_out[lb] = tot;
}

static EnvSwitch g_stepbuild{"MGCR_STEPBUILD"}, g_start_build{"MGCR_START_BUILD"};
static EnvSwitch g_sb_keep_all{"MGCR_SB_KEEP_ALL"};   // off: the step_build_kernel dispatch below
static EnvSwitch g_sb_real{"MGCR_SB_REAL"};            // the REALC instantiations
bool stepbuild_is_enabled() { return g_stepbuild.on(); }
bool set_stepbuild_enabled(bool on) { return g_stepbuild.set(on); }
bool set_start_build_enabled(bool on) { return g_start_build.set(on); }
bool set_stepbuild_keep_all_enabled(bool on) { return g_sb_keep_all.set(on); }
static int64_t g_stepbuild_launches = 0;
int64_t stepbuild_launch_count() { return g_stepbuild_launches; }
static int64_t g_keep_wide_launches = 0;   // ... of them, step_keep_wide_kernel
int64_t stepbuild_keep_wide_launch_count() { return g_keep_wide_launches; }
static int64_t g_apply_own_launches = 0;   // ... of them, keep forms whose apply takes the own r from the diagonal gather (sb_apply_form 1, 2)
int64_t stepbuild_apply_own_launch_count() { return g_apply_own_launches; }
static int64_t g_pair_launches = 0;        // ... of them, launched as step_pair_kernel (gcr_steppair.hip) or, at 3 and 4 directions, its late-r form
int64_t stepbuild_pair_launch_count() { return g_pair_launches; }
static int64_t g_pair_late_launches = 0;   // ... of them, launched as step_pair_late_kernel (gcr_steppair_late.hip), the close at 5 included
int64_t stepbuild_pair_late_launch_count() { return g_pair_late_launches; }

// The instantiation a step with `nd` stored directions launches (sb_kernel).
// KEEP-ALL (step_keep_kernel) where an instantiation keeps 0 scratch and 8 waves per SIMD: up to 2 stored directions in every
// form, 3 except the closing step with XR (tests/test_stepbuild_keep_all_regs.py).  With more directions the kept rows spill (the
// build's two trips of NDT streams, beta and the kept rows exceed 64 VGPRs): sb_keep_wide below, or step_build_kernel.
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_keep_fits() { return NDT <= 2 || (NDT == 3 && !(XR && CLOSE)); }
// (*form: the apply form of the instantiation, sb_apply_form)
template <int NDT, bool XR, bool CLOSE, bool R> const void *sb_keep(int *form) {
    *form = sb_apply_form<false, NDT, XR, CLOSE, R>();
    if constexpr (sb_keep_fits<NDT, XR, CLOSE>()) return (const void *)step_keep_kernel<NDT, XR, CLOSE, R>;
    else return nullptr;
}
// ... and step_keep_wide_kernel — the same body one trip at a time — where it has 0 scratch and 8 waves per SIMD
// (tests/test_stepbuild_keep_wide_regs.py) AND was measured faster than the step_build_kernel form it replaces: 4 stored directions
// with XR, inside a cycle and closing one (restart 4), and the close at 5 with and without XR.  At 4 directions without XR the
// in-cycle form was measured no faster (62.1 against 61.7 us at 128^3) and the closing one not at all: step_build_kernel, as for
// 5 directions inside a cycle (restart > 5).
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_keep_wide_fits() { return (NDT == 4 && XR) || (NDT == 5 && CLOSE); }
template <int NDT, bool XR, bool CLOSE, bool R> const void *sb_keep_wide_form(int *form) {
    *form = sb_apply_form<true, NDT, XR, CLOSE, R>();
    if constexpr (sb_keep_wide_fits<NDT, XR, CLOSE>()) return (const void *)step_keep_wide_kernel<NDT, XR, CLOSE, R>;
    else return nullptr;
}
static const void *sb_keep_wide(int nd, bool xr, bool close, bool realc, int *form) {
#define SKR(NDT, R) (close ? (xr ? sb_keep_wide_form<NDT, true, true, R>(form) : sb_keep_wide_form<NDT, false, true, R>(form)) \
                           : (xr ? sb_keep_wide_form<NDT, true, false, R>(form) : sb_keep_wide_form<NDT, false, false, R>(form)))
#define SKK(NDT) (realc ? SKR(NDT, true) : SKR(NDT, false))
    return nd == 4 ? SKK(4) : nd == 5 ? SKK(5) : nullptr;
#undef SKK
#undef SKR
}
// `mid`: the stencil view's middle slots are the row and its two neighbours (sten_lane_middle) — a keep form whose apply builds on that
// (sb_apply_form 1 and 2) is handed out only then; any other 7-slot view takes step_build_kernel: the same bits.
// *wide / *own (may be null): was it step_keep_wide_kernel, is its apply form 1 or 2?
static const void *sb_kernel(int nd, bool xr, bool close, bool realc, bool mid, bool *wide = nullptr, bool *own = nullptr) {
    if (wide) *wide = false;
    if (own) *own = false;
    const void *keep = nullptr;
    int form = 0;
    if (g_sb_keep_all.on() && nd > 3) keep = sb_keep_wide(nd, xr, close, realc, &form);
    if (g_sb_keep_all.on() && nd <= 3) {
#define SKR(NDT, R) (close ? (xr ? sb_keep<NDT, true, true, R>(&form) : sb_keep<NDT, false, true, R>(&form)) \
                           : (xr ? sb_keep<NDT, true, false, R>(&form) : sb_keep<NDT, false, false, R>(&form)))
#define SKK(NDT) (realc ? SKR(NDT, true) : SKR(NDT, false))
        keep = nd == 1 ? SKK(1) : nd == 2 ? SKK(2) : SKK(3);   // (nullptr: a form that does not fit, sb_keep_fits)
#undef SKK
#undef SKR
    }
    if (keep && (form == 0 || mid)) {
        if (wide) *wide = nd > 3;
        if (own) *own = form >= 1;
        return keep;
    }
#define SBR(NDT, R) (close ? (xr ? (const void *)step_build_kernel<3, 7, NDT, true, true, R> : (const void *)step_build_kernel<3, 7, NDT, false, true, R>) \
                           : (xr ? (const void *)step_build_kernel<3, 7, NDT, true, false, R> : (const void *)step_build_kernel<3, 7, NDT, false, false, R>))
#define SBK(NDT) (realc ? SBR(NDT, true) : SBR(NDT, false))
    switch (nd) {
        case 1: return SBK(1);
        case 2: return SBK(2);
        case 3: return SBK(3);
        case 4: return SBK(4);
        default: return SBK(5);
    }
#undef SBK
#undef SBR
}
// Do `grid` workgroups of this instantiation, with this much dynamic LDS, fit the chip AT ONCE?  The workgroups wait for each
// other inside the launch, so the answer has to come from the runtime (registers and LDS of the code object that was actually
// built: another compiler, -DMGCR_RES_TIMING, ... change them), not from arithmetic on what the kernel is meant to need.
// Asked once per instantiation and LDS size.  (What the runtime cannot know — CUs held by another process — is what the bounded
// polls and gcr_run's repeat are for.)
bool launch_is_coresident(const void *kernel, int threads, size_t dyn_lds, int grid) {
    struct Key { const void *k; size_t lds; int threads; int per_cu; };
    static std::vector<Key> seen;
    int per_cu = -1;
    for (const Key &e : seen)
        if (e.k == kernel && e.lds == dyn_lds && e.threads == threads) per_cu = e.per_cu;
    if (per_cu < 0) {
        if (dyn_lds > 0) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(dyn_lds > 64 * 1024 ? dyn_lds : 64 * 1024));
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, dyn_lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
        per_cu = nb;
        seen.push_back(Key{kernel, dyn_lds, threads, per_cu});
    }
    static const int force = getenv("MGCR_TEST_OCCUPANCY") ? atoi(getenv("MGCR_TEST_OCCUPANCY")) : -1;   // tests: pretend the runtime said so
    if (force >= 0) per_cu = force;
    return exchange_shared_init() == MGCR_OK && (int64_t)per_cu * exchange_shared().cus >= grid;
}

static size_t sb_lds_bytes(const CsrDev &A, int g) {
    return sizeof(cplx) * RED_THREADS * (size_t)((A.nrow + (int64_t)g * RED_THREADS - 1) / ((int64_t)g * RED_THREADS));
}

// can step `lim` of a lean cycle on A run as one launch?  (single GPU, 7-slot stencil view, <= 5 stored directions, A r in LDS)
bool csr_step_build_eligible(const CsrDev &A, const DistCsr *dist, int lim) {
    if (!g_stepbuild.on() || dist || comm_live_count() > 0 || lim < 1 || lim > SB_MAX_ND) return false;
    if (!csr_fusable(A, nullptr) || !csr_stencil_active(A) || A.sten_rare || sten_slots(A) != 7) return false;
    const int g = red_grid(A.nrow);
    if (g < 64 || g % 8 != 0) return false;   // (smaller systems have the resident solver or the xr-fused kernels)
    if ((int64_t)g * RED_THREADS * SB_MAX_TRIPS < A.nrow) return false;
    if (A.reach >= FUSED_TILE_REACH_DEFAULT) return false;   // rows that reach this far take the LDS-window kernels (gcr_fused.hip)
    if (exchange_shared_init() != MGCR_OK) return false;
    if (g > RES_BLK) return false;
    // every form the step may be launched in (with / without the next residual update, closing or not) must be co-resident
    const size_t lds = sb_lds_bytes(A, g);
    const bool realc = g_sb_real.on() && row_mat(A, false, cplx{0., 0.}).realv;
    for (int xr = 0; xr < 2; xr++)
        for (int cl = 0; cl < 2; cl++)
            if (!launch_is_coresident(sb_kernel(lim, xr != 0, cl != 0, realc, sten_lane_middle(A)), RED_THREADS, lds, g)) return false;
    return true;
}

// the members the kernels share; `ngen`: exchange generations the launch may use
template <class Args>
static int sb_fill_common(Args &a, const CsrDev &A, bool shift, cplx k, DevState *st, const RowMap &rm, unsigned ngen) {
    MGCR_TRY(exchange_shared_init());
    const ExchangeShared &sh = exchange_shared();
    a.m = row_mat(A, shift, k);
    a.n = A.nrow;
    a.nlogical = red_grid(A.nrow);
    a.rm = rm;
    a.st = st;
    a.slots = sh.slots; a.abort_dev = sh.abort_dev; a.abort_host = sh.abort_host;
    a.gen0 = exchange_take_generations(ngen);
    a.test_stall = getenv("MGCR_TEST_STEPBUILD_STALL") ? atoi(getenv("MGCR_TEST_STEPBUILD_STALL")) : 0;
    a.spin_limit = getenv("MGCR_TEST_RESIDENT_SPIN_LIMIT") ? atoi(getenv("MGCR_TEST_RESIDENT_SPIN_LIMIT")) : RES_SPIN_LIMIT;
    return MGCR_OK;
}
static int sb_launch(const void *kernel, void *args, int grid, size_t lds_bytes, const char *who) {
    MGCR_CHECK(launch_is_coresident(kernel, RED_THREADS, lds_bytes, grid), MGCR_ERR_INVALID, "%s: launch would not be co-resident", who);
    void *kargs[1] = {args};
    MGCR_HIP(hipLaunchKernel(kernel, dim3((unsigned)grid), dim3(RED_THREADS), kargs, lds_bytes, ctx().stream));
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

int csr_step_build(const CsrDev &A, const cplx *x, bool shift, cplx k, const cplx *const *aps, int nd, DevState *st, int it, const double *partsR,
                   int nblkR, int strideR, double *hist, int hist_cap, const cplx *den, cplx *ap_out, double *partsA, LeanCoef *lc,
                   const RowMap &rm, cplx *xr_out, cplx *xr_den_slot, int xr_slot, double *partsR_out, const cplx *const *close_ps, cplx *close_p_out,
                   cplx *close_x) {
    MGCR_CHECK(nd >= 1 && nd <= SB_MAX_ND, MGCR_ERR_INVALID, "csr_step_build: 1..5 directions");
    StepBuildArgs a;
    MGCR_TRY(sb_fill_common(a, A, shift, k, st, rm, 3));
    a.x = x;
    for (int j = 0; j < SB_MAX_ND; j++) a.aps[j] = aps[j < nd ? j : 0];
    a.it = it; a.partsR = partsR; a.nblkR = nblkR; a.strideR = strideR; a.hist = hist; a.hist_cap = hist_cap;
    a.den = den; a.ap_out = ap_out; a.partsA = partsA; a.lc = lc;
    for (int j = 0; j < SB_MAX_ND; j++) a.ps[j] = close_ps ? close_ps[j < nd ? j : 0] : nullptr;
    a.p_out = close_p_out; a.xvec = close_x;
    a.xr_out = xr_out; a.xr_den_slot = xr_den_slot; a.xr_slot = xr_slot; a.partsR_out = partsR_out;
    const bool xr = xr_out != nullptr, close = close_ps != nullptr, realc = g_sb_real.on() && a.m.realv;
    bool wide, own;
    const void *kernel = sb_kernel(nd, xr, close, realc, sten_lane_middle(A), &wide, &own);
    // The pair form (gcr_steppair.hip) of a keep step whose apply takes the own r from the diagonal gather: one workgroup per CU
    // carries two of the 512 logical ones.  Built for the operator itself, not for 1 - k A (a DiracOp keeps the keep forms).  Asked per
    // launch like everything above; where it does not fit, the keep form runs.
    const bool pair_ok = own && !shift && g_sb_keep_all.on() && a.nlogical == SB_PAIR_LOGICAL && exchange_shared().cus >= SB_PAIR_GRID;
    const void *pair = pair_ok ? sb_pair_kernel(nd, xr, close, realc) : nullptr;
    // Its late-r form (gcr_steppair_late.hip) loads r again from a.x in the build: a.x must be a vector the launch does not write.
    // The drivers hand in a residual of the ring that is neither the next one nor a direction; where that does not hold, the forms
    // above run.
    const void *late = pair_ok && a.x != a.xr_out && a.x != a.p_out ? sb_pair_late_kernel(nd, xr, close, realc) : nullptr;
    if (late && launch_is_coresident(late, RED_THREADS, SB_PAIR_LDS, SB_PAIR_GRID)) {
        MGCR_TRY(sb_launch(late, &a, SB_PAIR_GRID, SB_PAIR_LDS, "csr_step_build (late-r pair form)"));
        g_pair_late_launches++;
        if (!close) g_pair_launches++;   // (a pair step at 1..4 directions, whichever of the two kernels ran it)
    } else if (pair && launch_is_coresident(pair, RED_THREADS, SB_PAIR_LDS, SB_PAIR_GRID)) {
        MGCR_TRY(sb_launch(pair, &a, SB_PAIR_GRID, SB_PAIR_LDS, "csr_step_build (pair form)"));
        g_pair_launches++;
    } else {
        MGCR_TRY(sb_launch(kernel, &a, a.nlogical, sb_lds_bytes(A, a.nlogical), "csr_step_build"));
    }
    // (the three counters below count steps by FORM, whichever kernel ran it: a pair form is a one-launch step, reads r once and
    // takes its own r from the diagonal gather)
    g_stepbuild_launches++;
    if (wide) g_keep_wide_launches++;
    if (own) g_apply_own_launches++;
    return MGCR_OK;
}

static int64_t g_start_build_launches = 0;
int64_t start_build_launch_count() { return g_start_build_launches; }
static const void *start_kernel(bool realc) {
    return realc ? (const void *)start_build_kernel<true> : (const void *)start_build_kernel<false>;
}

// can the start of a solve on A run as one launch?  (the conditions of a one-launch step, and its own kernel co-resident)
bool csr_start_build_eligible(const CsrDev &A, const DistCsr *dist) {
    if (!g_start_build.on() || !csr_step_build_eligible(A, dist, 1)) return false;
    const bool realc = g_sb_real.on() && row_mat(A, false, cplx{0., 0.}).realv;
    return launch_is_coresident(start_kernel(realc), RED_THREADS, sb_lds_bytes(A, red_grid(A.nrow)), red_grid(A.nrow));
}

int csr_start_build(const CsrDev &A, const cplx *b, bool shift, cplx k, cplx *ap0, DevState *st, double *hist, LeanCoef *lc, cplx *den0,
                    cplx *r_out, double *partsR_out, const RowMap &rm) {
    StartArgs a;
    MGCR_TRY(sb_fill_common(a, A, shift, k, st, rm, 1));
    a.b = b;
    a.ap0 = ap0;
    a.hist = hist; a.lc = lc; a.den0 = den0; a.r_out = r_out; a.partsR_out = partsR_out;
    MGCR_TRY(sb_launch(start_kernel(g_sb_real.on() && a.m.realv), &a, a.nlogical, sb_lds_bytes(A, a.nlogical), "csr_start_build"));
    g_start_build_launches++;
    return MGCR_OK;
}

}  // namespace mgcr
