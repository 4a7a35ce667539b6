// The PAIR form of a one-launch GCR step (gcr_stepbuild.hip, gcr_stepbuild_keep_body.h): one physical workgroup of 1024 threads per
// CU — grid 256, up to 128 VGPRs, 4 waves per SIMD — carries TWO logical workgroups of the keep forms' launch, the two that ran on
// that XCD as physical workgroups p1 = ((b >> 3) << 4) | (b & 7) and p1 + 8 of its grid of 512.
// Why: the keep forms run two workgroups per CU at 64 VGPRs, of which 32-40 are the working set (stream batches, offsets,
// accumulators) and are paid per thread; of a thread's 4 rows of Ap_0 1 to 3 survive in registers from the pass-1 dots to the build,
// the others are read from memory twice.  Here a thread owns the 2 x 4 rows the two logical workgroups gave thread `tid`, holds the
// working set once, and keeps ALL eight rows of Ap_0 — and rows of Ap_1 where a form has registers left (sb_pair_kept) — across
// exchange 1.  A r of the eight rows lives in LDS (128 KB dynamic).
// The bits are the keep forms': every sum keeps its operands, its order and its tree.
//   * Per logical workgroup a thread accumulates over ITS four rows in trip order; a wave's trees run the two logical workgroups'
//     sums side by side (wave_multi_sum sums every scalar by the same tree whatever their number: reduce.h), and the waves' sums
//     are added in wave order per logical workgroup.  No row of one is added into a sum of the other.
//   * Two slots are published per exchange, two entries each written to partsA and partsR_out, indexed by LOGICAL number: nothing
//     downstream sees the pairing.  The hop-1 tasks of both logical numbers are folded here, on different waves (sp_collect).
//   * The scalar stage's writes go out once, from the physical workgroup that carries logical workgroup 0.
//   * |r|^2 of the step before is one value for everybody: folded once per physical workgroup.
// Built for real coefficients and an operator without a shift (A itself, not 1 - k A), with the next residual update: in-cycle
// steps at 1..4 stored directions and the close at 5 — the five kernels of the restart-5 headline.  Handed out by default: 2, 3 and
// 4 directions (sb_pair_form: the forms whose own trace cleared the gate).  Everything else keeps its kernel.
// Needs >= 256 CUs and 512 logical workgroups (gcr_stepbuild.hip csr_step_build asks; option step_build_pair, MGCR_SB_PAIR).
#include "internal.h"
#include "reduce.h"
#include "gcr_dev.h"
#include "spmv_dev.h"
#include "exchange_dev.h"
#include "gcr_stepbuild_dev.h"

namespace mgcr {

constexpr int SP_ROWS = 2 * SB_MAX_TRIPS;   // thread-rows: u < SB_MAX_TRIPS logical workgroup A's trip u, the others B's trip u - SB_MAX_TRIPS
// Thread-rows kept in registers from the pass-1 dots to the build: the LAST rows pass 1 loads — it walks the directions last to
// first — i.e. the eight rows of Ap_0, then rows of Ap_1 (its first ones: the build meets them first).  Per form the most with which
// it compiles to 0 scratch, <= 128 VGPRs and 4 waves per SIMD (tests/test_stepbuild_pair_regs.py pins table and resources):
//   form                     kept (Ap_0 + Ap_1)   VGPRs   one row more
//   1 direction               8  (8 + 0)           106     (there is no other row)
//   2 directions             15  (8 + 7)           128     16 B of scratch per lane
//   3 directions             14  (8 + 6)           128     36 B
//   4 directions             11  (8 + 3)           125     8 B
//   the close at 5           12  (8 + 4)           128     20 B
// (two rows per batch of the build, eight loads per direction in flight in pass 1; with four rows per batch of the build the forms
// at 4 and 5 directions need 36 and 100 B with the eight rows of Ap_0 alone.)
// -DMGCR_SB_PAIR_KEPT=K builds K (<= 16) for every form with more than one direction, for such a derivation.
#ifndef MGCR_SB_PAIR_KEPT
#define MGCR_SB_PAIR_KEPT -1
#endif
template <int NDT, bool CLOSE> constexpr int sb_pair_kept() {
    if (NDT == 1) return SP_ROWS;
    if (MGCR_SB_PAIR_KEPT >= 0) return MGCR_SB_PAIR_KEPT;
    return NDT == 2 ? 15 : NDT == 3 ? 14 : NDT == 4 ? 11 : 12;
}
// Rows per batch of the pass-1 loads: 8 keeps the 128 KB of a direction per CU in flight that the keep forms have, 4 halves it —
// measured the same (298.7 / 297.2 against 298.9 / 299.6 us per cycle), 8 stays.  Rows per batch of the build and of the close pass:
// 2 (with 4 the forms at 4 and 5 directions spill, see above).
#ifndef MGCR_SB_PAIR_P1
#define MGCR_SB_PAIR_P1 8
#endif
#ifndef MGCR_SB_PAIR_TB
#define MGCR_SB_PAIR_TB 2
#endif
// 1: the next residual r' leaves with streaming stores (st_stream) instead of plain ones, so that less of it sits dirty in the L2s
// when the launch ends.  Measured slower in every form (310.0 / 312.9 against 298.7 / 297.2 us per cycle: the next launch's gathers
// of r' lose their L2 hits): not built.
#ifndef MGCR_SB_PAIR_XR_STREAM
#define MGCR_SB_PAIR_XR_STREAM 0
#endif
// The forms the default dispatch launches: those whose own kernel trace showed them faster than the keep form they replace by
// more than the rows' standard deviations.  -DMGCR_SB_PAIR_FORMS=1 / 0 hands out all / none, for a measurement.
#ifndef MGCR_SB_PAIR_FORMS
#define MGCR_SB_PAIR_FORMS -1
#endif
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_pair_built() { return XR && (CLOSE ? NDT == 5 : NDT <= 4); }
template <int NDT, bool XR, bool CLOSE> constexpr bool sb_pair_form() {
    if (!sb_pair_built<NDT, XR, CLOSE>()) return false;
    if (MGCR_SB_PAIR_FORMS >= 0) return MGCR_SB_PAIR_FORMS != 0;
    // 2, 3 and 4 directions: 3.3 to 4.5 us faster than their keep forms at 128^3, the rows' standard deviations 0.6 to 2.2 us.  At 1
    // direction 2.0 us with standard deviations of 1.3 to 2.5 us, at the close 0.2 us with 1.2 to 1.4 us: not handed out.
    return !CLOSE && NDT >= 2;
}

// The wave trees of 2 x H per-thread sums, v[0..H) logical workgroup A's and v[H..2H) B's: lds[w][(k0 + k) * 17 + wave] gets what
// block_sum_owner<NV> / sb_wave_pair_to_lds put there in a workgroup that is logical workgroup w alone.
template <int H, int LN>
__device__ __forceinline__ void sp_wave_sums_to_lds(double (&v)[2 * H], double (&lds)[2][LN], int k0) {
    static_assert(H == 1 || H == 2 || H == 4, "2 H scalars: a power of two, every lane group owns one");
    double s;
    const int k = wave_multi_sum<2 * H>(v, s);
    if (((int)threadIdx.x & (64 / (2 * H) - 1)) == 0) lds[k / H][(k0 + k % H) * 17 + ((int)threadIdx.x >> 6)] = s;
}
// ... and the waves' sums added in wave order: thread k of wave w < 2 returns logical workgroup w's total of scalar k < NV (the
// others 0.).  `lds` must not be reused before another barrier.
template <int NV, int LN>
__device__ __forceinline__ double sp_block_owner_from_lds(const double (&lds)[2][LN]) {
    __syncthreads();
    const int w = (int)threadIdx.x >> 6, k = (int)threadIdx.x & 63;
    double t = 0.;
    if (w < 2 && k < NV)
        for (int q = 0; q < RED_THREADS / 64; q++) t += lds[w][k * 17 + q];
    return t;
}

// One bounded poll of exchange_dev.h: the value of the {value, generation} slot at byte `at` once it carries `want`; gives up
// (flag in LDS, 0.) like res_collect's polls.
__device__ __forceinline__ double sp_poll(ResSync &s, int at, unsigned want) {
    int spins = 0;
    for (;;) {
        const v4i w = __builtin_amdgcn_raw_buffer_load_b128(s.slots, at, 0, RES_SC1);
        if ((unsigned)w.z == want) return __hiloint2double(w.y, w.x);
        spins++;
        if (spins > s.spin_limit || ((spins & 255) == 0 && __hip_atomic_load(s.abort_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            *s.gave_up = 1;
            return 0.;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
// res_collect (exchange_dev.h) for a physical workgroup that carries two logical ones.  The hop-1 tasks are indexed by logical
// workgroup and wave, task = wave * nblk + lb: this workgroup takes those of both its logical numbers, lbs[w & 1] on its waves w
// (as that workgroup's wave w >> 1, w >> 1 + 8, ...) — which wave folds a task does not enter its sum.  Hop 2 and the totals are
// res_collect's (the copy is logical workgroup lbs[0]'s, s.lb); the generation advances once.  Kept apart from res_collect: written as one
// function with the number of logical workgroups as a parameter, the existing kernels' instruction order changes.
template <int NVT>
__device__ __forceinline__ bool sp_collect(ResSync &s, int kind, const int (&lbs)[2]) {
    static_assert(NVT <= RES_NV, "scalars per exchange");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ng = (s.nblk + 63) >> 6;   // groups that hold workgroups
    for (int task = (wave >> 1) * s.nblk + lbs[wave & 1]; task < ng * NVT; task += (RED_THREADS / 128) * s.nblk) {   // wave-uniform
        const int g = task / NVT, k = task - g * NVT;
        const int blk = g * 64 + lane;
        const double v = blk < s.nblk ? sp_poll(s, ((kind * RES_NV + k) * RES_BLK + blk) * 16, s.gen) : 0.;
        double t = wave_sum(v);
        t = __shfl(t, 0, 64);
        if (lane < RES_COPIES) {
            const v4i w4 = {__double2loint(t), __double2hiint(t), (int)s.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, s.slots, RES_L2_BASE + ((lane * 3 + kind) * RES_NV + k) * RES_GRP * 16 + g * 16, 0, RES_SC1);
        }
    }
    if ((int)threadIdx.x < RES_GRP * NVT) {
        const int k = (int)threadIdx.x / RES_GRP, g = (int)threadIdx.x % RES_GRP;
        const int copy = s.lb & (RES_COPIES - 1);
        s.ws[k * RES_GRP + g] = g < ng ? sp_poll(s, RES_L2_BASE + ((copy * 3 + kind) * RES_NV + k) * RES_GRP * 16 + g * 16, s.gen) : 0.;
    }
    __syncthreads();
    s.gen++;
    return *s.gave_up == 0;
}

template <int NDT, bool CLOSE>
__global__ void __launch_bounds__(RED_THREADS, 4) step_pair_kernel(StepBuildArgs a) {
    constexpr int KT = sb_pair_kept<NDT, CLOSE>();
    constexpr int K0 = KT < SP_ROWS ? KT : SP_ROWS, K1 = NDT >= 2 && KT > SP_ROWS ? KT - SP_ROWS : 0;   // rows of Ap_0, of Ap_1
    static_assert(KT >= 0 && KT <= 2 * SP_ROWS, "rows of Ap_0 and Ap_1");
    constexpr int P1 = MGCR_SB_PAIR_P1, TB = MGCR_SB_PAIR_TB;
    static_assert(SP_ROWS % P1 == 0 && SP_ROWS % TB == 0, "whole batches");
    constexpr int SB_STAGE_N = CLOSE ? 2 * NDT + NDT * NDT : NDT;
    constexpr int LN = (2 * NDT > 4 ? 2 * NDT : 4) * 17;
    __shared__ double lds[2][LN];   // one set of wave sums per logical workgroup
    __shared__ double lds_pw[2 * SB_MAX_ND * 17], lds_ws[2 * SB_MAX_ND * RES_GRP];
    __shared__ int gave_up;
    __shared__ cplx sbeta[NDT], scp[NDT];
    __shared__ double lds_rr[17];
    __shared__ cplx sstg[SB_STAGE_N];
    extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];   // Ar of this workgroup's rows: [thread-row][thread]
    if (a.st->stop_at < a.st->base + a.it) return;
    const int p1 = (((int)blockIdx.x >> 3) << 4) | ((int)blockIdx.x & 7);
    const int lbs[2] = {logical_workgroup(a.rm, p1, a.nlogical), logical_workgroup(a.rm, p1 + 8, a.nlogical)};
    if (lbs[0] >= a.nlogical || lbs[1] >= a.nlogical) return;
    const bool has0 = lbs[0] == 0 || lbs[1] == 0;   // carries logical workgroup 0: the scalar stage's writes
    cplx *arL = reinterpret_cast<cplx *>(sb_smem);
    const int tid = (int)threadIdx.x;
    const int own_w = tid >> 6, own_k = tid & 63;    // the owner of logical workgroup own_w's total of scalar own_k (own_w < 2)
    const int own_lb = lbs[own_w & 1];
    ResSync sy;
    res_sync_init(sy, a.slots, a.gen0, a.nlogical, lbs[0], a.abort_dev, a.spin_limit, lds_pw, lds_ws, &gave_up);
    if (a.test_stall && (lbs[0] == a.test_stall - 1 || lbs[1] == a.test_stall - 1)) return;
    int64_t i0[2], end[2], stride, stride_b;
    row_range(a.rm, lbs[0], a.nlogical, a.n, &i0[0], &end[0], &stride);
    row_range(a.rm, lbs[1], a.nlogical, a.n, &i0[1], &end[1], &stride_b);   // (the step is the map's: the same)
    auto row = [&](int u) -> int64_t { return i0[u / SB_MAX_TRIPS] + (int64_t)(u % SB_MAX_TRIPS) * stride; };
    auto live = [&](int u) -> bool { return row(u) < end[u / SB_MAX_TRIPS]; };
    uint32_t off[SP_ROWS];   // the rows' byte offsets (n < 2^28 rows here): every stream is scalar base + this
#pragma unroll
    for (int u = 0; u < SP_ROWS; u++) off[u] = (uint32_t)row(u) * (uint32_t)sizeof(cplx);
    auto at = [&](auto *p, int u) { return sb_elem(p, off[u]); };
    cplx rk[SP_ROWS];   // r of the thread's rows, from the apply to the last pass
    // ---- apply: Ar to LDS, r kept (the keep body's apply with the own r from the diagonal gather, sb_apply_form 1) ----
#pragma unroll
    for (int u = 0; u < SP_ROWS; u++) {
        const int64_t i = row(u), e = end[u / SB_MAX_TRIPS];
        rk[u] = make_double2(0., 0.);
        const auto xj = [&](int32_t j) -> cplx { return *sb_elem(a.x, (uint32_t)j * (uint32_t)sizeof(cplx)); };
        // (a whole wave enters, also its lanes beyond `end`: a wave's rows are 64 consecutive ones from a multiple of 64)
        if (__builtin_amdgcn_readfirstlane((int32_t)i) < (int32_t)e) {
            cplx own;
            const cplx sum = sten_row_product_own_t<1, false>(a.m, i, xj, own);
            if (i < e) {
                rk[u] = own;
                arL[u * RED_THREADS + tid] = sum;   // (no shifted operator here: csr_step_build asks)
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // (one row's gathers in registers at a time)
    }
    // the scalar stage's operands, requested behind the apply and parked in LDS (see the keep body); every pair form carries the
    // next residual update, so every workgroup folds |r|^2
    {
        const double stg_r = a.nblkR == 1 ? (tid == 0 ? a.partsR[0] + 0. : 0.) : (tid < a.nblkR ? a.partsR[tid] : 0.);
        cplx stg_c = make_double2(0., 0.);
        const int stg_i = tid - (RED_THREADS - 64);
        if (stg_i >= 0 && stg_i < SB_STAGE_N) stg_c = *sb_stage_src<NDT>(a.den, a.lc, stg_i);
        sb_stage_rr_waves(stg_r, a.nblkR, lds_rr);
        if (stg_i >= 0 && stg_i < SB_STAGE_N) sstg[stg_i] = stg_c;
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- <Ar, Ap_j> per logical workgroup, one direction (all rows) at a time, last direction first; the kept rows stay ----
    cplx pre0[K0 > 0 ? K0 : 1], pre1[K1 > 0 ? K1 : 1];
    {
#pragma unroll
        for (int jj = 0; jj < NDT; jj++) {
            const int j = NDT - 1 - jj;
            double v[4] = {0., 0., 0., 0.};   // A's pair, B's pair
#pragma unroll
            for (int u0 = 0; u0 < SP_ROWS; u0 += P1) {
                cplx b[P1];
#pragma unroll
                for (int q = 0; q < P1; q++) b[q] = live(u0 + q) ? ld_stream<true>(at(a.aps[j], u0 + q)) : make_double2(0., 0.);
#pragma unroll
                for (int q = 0; q < P1; q++) {
                    const int u = u0 + q;
                    if (live(u)) {
                        const cplx tt = cconj_mul(arL[u * RED_THREADS + tid], b[q]);
                        v[2 * (u / SB_MAX_TRIPS)] += tt.x;
                        v[2 * (u / SB_MAX_TRIPS) + 1] += tt.y;
                    }
                    if (j == 0 && u < K0) pre0[u < K0 ? u : 0] = b[q];
                    if (j == 1 && u < K1) pre1[u < K1 ? u : 0] = b[q];
                }
                if (P1 < SP_ROWS) __builtin_amdgcn_sched_barrier(0);
            }
            sp_wave_sums_to_lds<2>(v, lds, 2 * j);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double mine = sp_block_owner_from_lds<2 * NDT>(lds);
        if (own_w < 2 && own_k < 2 * NDT) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((1 * RES_NV + own_k) * RES_BLK + own_lb) * 16, 0, RES_SC1);
        }
    }
    // the stop decision, ahead of the poll (the barrier above has made lds_rr visible); in a scalar register from here on
    const bool ends_here = __builtin_amdgcn_readfirstlane(!((sb_stage_rr(a.nblkR, lds_rr) / a.st->bnorm2) > a.st->tol2)) != 0;
    if (!sp_collect<2 * NDT>(sy, 1, lbs)) {
        res_abort(a.abort_dev, a.abort_host);
#pragma unroll
        for (int u = 0; u < SP_ROWS; u++)
            if (live(u)) *at(a.ap_out, u) = make_double2(__builtin_nan(""), __builtin_nan(""));
        if (own_w < 2 && own_k < 4) a.partsA[own_k * RED_MAX_BLOCKS + own_lb] = __builtin_nan("");
        return;
    }
    // ---- the scalar stage's arithmetic and writes, then the direction build ----
    if (has0 && tid == 0) {
        close_step(a.st, a.it, sb_stage_rr(a.nblkR, lds_rr), a.hist, a.hist_cap, CLOSE);
        if (CLOSE) a.st->closed = 1;
    }
    if (tid < NDT) sbeta[tid] = cdiv(make_double2(res_total(sy, 2 * tid), res_total(sy, 2 * tid + 1)), sstg[tid]);
    __syncthreads();
    if constexpr (CLOSE) {
        if (tid < NDT) scp[tid] = sb_stage_close_coef<NDT>(sstg + 2 * NDT + tid * NDT, sbeta, tid);
        __syncthreads();
    }
    if (!CLOSE && has0 && tid <= NDT) lean_table_row<NDT>(a.lc, sbeta, tid);
    {
        cplx beta[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) beta[j] = to_sgpr(sbeta[j]);
        double v[8] = {0., 0., 0., 0., 0., 0., 0., 0.};   // A's <r,Ap'>, <Ap',Ap'>, then B's
#pragma unroll
        for (int u0 = 0; u0 < SP_ROWS; u0 += TB) {
            cplx ac[TB];
#pragma unroll
            for (int q = 0; q < TB; q++) ac[q] = make_double2(0., 0.);
#pragma unroll
            for (int j = 0; j < NDT; j++) {   // (j = 0 .. NDT - 1 for every row, from a register where the row is kept)
                cplx aj[TB];
#pragma unroll
                for (int q = 0; q < TB; q++) {
                    const int u = u0 + q;
                    aj[q] = (j == 0 && u < K0)   ? pre0[u < K0 ? u : 0]
                            : (j == 1 && u < K1) ? pre1[u < K1 ? u : 0]
                            : live(u)            ? ld_stream<NTS>(at(a.aps[j], u))
                                                 : make_double2(0., 0.);
                }
#pragma unroll
                for (int q = 0; q < TB; q++) ac[q] = csub(ac[q], cmul(beta[j], aj[q]));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < TB; q++) {
                const int u = u0 + q, h = 4 * (u / SB_MAX_TRIPS);
                if (live(u)) {
                    const cplx an = cadd(arL[u * RED_THREADS + tid], ac[q]);
                    *at(a.ap_out, u) = an;
                    arL[u * RED_THREADS + tid] = an;   // (A r is not needed any more; the update below wants Ap')
                    const cplx tt = cconj_mul(rk[u], an);
                    v[h] += tt.x; v[h + 1] += tt.y;
                    const cplx w = cconj_mul(an, an);
                    v[h + 2] += w.x; v[h + 3] += w.y;
                }
            }
        }
        sp_wave_sums_to_lds<4>(v, lds, 0);
        const double mine = sp_block_owner_from_lds<4>(lds);
        if (own_w < 2 && own_k < 4) {
            a.partsA[own_k * RED_MAX_BLOCKS + own_lb] = mine;
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((2 * RES_NV + own_k) * RES_BLK + own_lb) * 16, 0, RES_SC1);
        }
    }
    if constexpr (CLOSE) {
        // x += sum_j cx_j p_j;  P0' = r - sum_j cp_j p_j  (p_0 = P0, p_m = D_m), while the exchange-2 partials travel
        cplx cx[NDT], cp[NDT];
#pragma unroll
        for (int j = 0; j < NDT; j++) {
            cx[j] = to_sgpr(sstg[NDT + j]);
            cp[j] = to_sgpr(scp[j]);
        }
#pragma unroll
        for (int u0 = 0; u0 < SP_ROWS; u0 += TB) {
            cplx xv[TB], pc[TB];
#pragma unroll
            for (int q = 0; q < TB; q++) {
                xv[q] = live(u0 + q) ? *at(a.xvec, u0 + q) : make_double2(0., 0.);
                pc[q] = make_double2(0., 0.);
            }
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx pj[TB];
#pragma unroll
                for (int q = 0; q < TB; q++) pj[q] = live(u0 + q) ? ld_stream<NTS>(at(a.ps[j], u0 + q)) : make_double2(0., 0.);
#pragma unroll
                for (int q = 0; q < TB; q++) {
                    xv[q] = cadd(xv[q], cmul(cx[j], pj[q]));
                    pc[q] = csub(pc[q], cmul(cp[j], pj[q]));
                }
            }
#pragma unroll
            for (int q = 0; q < TB; q++) {
                if (live(u0 + q)) {
                    *at(a.xvec, u0 + q) = xv[q];
                    st_stream<NTS>(at(a.p_out, u0 + q), cadd(rk[u0 + q], pc[q]));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- the next step's residual update ----
    if (!sp_collect<4>(sy, 2, lbs)) {
        res_abort(a.abort_dev, a.abort_host);
#pragma unroll
        for (int u = 0; u < SP_ROWS; u++)
            if (live(u)) *at(a.xr_out, u) = make_double2(__builtin_nan(""), __builtin_nan(""));
        if (own_w < 2 && own_k == 0) a.partsR_out[own_lb] = __builtin_nan("");
        return;
    }
    if (ends_here) return;
    const cplx alpha = sb_xr_alpha(sy, a.st, a.lc, a.xr_den_slot, a.xr_slot, has0 ? 0 : 1);
    double vr[2] = {0., 0.};
#pragma unroll
    for (int u = 0; u < SP_ROWS; u++) {
        if (live(u)) {
            const cplx rn = csub(rk[u], cmul(alpha, arL[u * RED_THREADS + tid]));
            st_stream<MGCR_SB_PAIR_XR_STREAM != 0>(at(a.xr_out, u), rn);
            vr[u / SB_MAX_TRIPS] += rn.x * rn.x + rn.y * rn.y;
        }
    }
    sp_wave_sums_to_lds<1>(vr, lds, 0);
    const double tot = sp_block_owner_from_lds<1>(lds);
    if (own_w < 2 && own_k == 0) a.partsR_out[own_lb] = tot;
}

static EnvSwitch g_sb_pair{"MGCR_SB_PAIR"};
bool set_stepbuild_pair_enabled(bool on) { return g_sb_pair.set(on); }

template <int NDT, bool XR, bool CLOSE> static const void *sb_pair_entry() {
    if constexpr (sb_pair_form<NDT, XR, CLOSE>()) return (const void *)step_pair_kernel<NDT, CLOSE>;
    else return nullptr;
}
const void *sb_pair_kernel(int nd, bool xr, bool close, bool realc) {
    if (!g_sb_pair.on() || !realc || !xr) return nullptr;
    if (close) return nd == 5 ? sb_pair_entry<5, true, true>() : nullptr;
    switch (nd) {
        case 1: return sb_pair_entry<1, true, false>();
        case 2: return sb_pair_entry<2, true, false>();
        case 3: return sb_pair_entry<3, true, false>();
        case 4: return sb_pair_entry<4, true, false>();
        default: return nullptr;
    }
}

}  // namespace mgcr
