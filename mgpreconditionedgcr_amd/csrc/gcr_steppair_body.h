// The body of the pair forms of a one-launch GCR step — gcr_steppair.hip step_pair_kernel and gcr_steppair_late.hip
// step_pair_late_kernel (see there): included INSIDE each kernel template, behind `using POL = SbPairPolicy<...>`
// (gcr_steppair_dev.h), with the template parameters NDT, CLOSE and the argument `a` in scope.  One text, two kernel names; not a
// header to include anywhere else.
// apply (Ar to LDS; r kept, or with POL::LATE_R dropped) | the scalar stage's operands requested and parked in LDS | pass-1 dots,
// KT rows of the stored directions kept | publish exchange 1, |r|^2 fold and stop decision | poll 1 | the stage's arithmetic and
// writes | build (LATE_R: r loaded again at the head of each batch) | CLOSE: close pass | poll 2, residual update.
    constexpr int KT = POL::KT;
    constexpr bool LATE_R = POL::LATE_R;
    constexpr int LATE_FROM = LATE_R ? POL::LATE_FROM : SP_ROWS;   // thread-rows u >= LATE_FROM load their r again in the build
    static_assert(KT >= 0 && KT <= NDT * SP_ROWS, "rows of Ap_0 .. Ap_{NDT - 1}");
    static_assert(LATE_FROM >= 0 && LATE_FROM <= SP_ROWS, "thread-rows");
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
    cplx rk[SP_ROWS];   // r of the thread's rows: from the apply to the last pass, rows u >= LATE_FROM from the build
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
                if (u < LATE_FROM) rk[u] = own;
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
    cplx pre[KT > 0 ? KT : 1];   // row u of Ap_j at j * SP_ROWS + u
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
                    const int k = j * SP_ROWS + u;
                    if (k < KT) pre[k < KT ? k : 0] = b[q];
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
            if constexpr (LATE_R) {   // r of the batch's rows, again: the lines the apply's gathers brought in (a plain load)
#pragma unroll
                for (int q = 0; q < TB; q++)
                    if (u0 + q >= LATE_FROM) rk[u0 + q] = live(u0 + q) ? *at(a.x, u0 + q) : make_double2(0., 0.);
            }
#pragma unroll
            for (int j = 0; j < NDT; j++) {   // (j = 0 .. NDT - 1 for every row, from a register where the row is kept)
                cplx aj[TB];
#pragma unroll
                for (int q = 0; q < TB; q++) {
                    const int u = u0 + q, k = j * SP_ROWS + u;
                    aj[q] = k < KT     ? pre[k < KT ? k : 0]
                            : live(u)  ? ld_stream<NTS>(at(a.aps[j], u))
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
