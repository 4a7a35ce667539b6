// The body of gcr_stepbuild.hip's step_keep_kernel and step_keep_wide_kernel (see there): included INSIDE each of the two kernel
// templates, behind `using POL = SbKeepPolicy<...>`, with the template parameters NDT, XR, CLOSE, REALC and the argument `a` in scope.
// One text, two kernel names; not a header to include anywhere else.
// apply (Ar to LDS, r kept) | the scalar stage's operands requested and parked in LDS | pass-1 dots, the first KT rows of Ap_0
// kept | publish exchange 1, |r|^2 fold and stop decision | poll 1 | the stage's arithmetic and writes | build | CLOSE: close pass
// | XR: poll 2, residual update.
    constexpr int TB = POL::TB, KT = POL::KT;
    constexpr int SB_STAGE_N = CLOSE ? 2 * NDT + NDT * NDT : NDT;
    constexpr bool OTF = POL::OTF;
    __shared__ double lds[(2 * NDT > 4 ? 2 * NDT : 4) * 17];
    __shared__ double lds_pw[2 * SB_MAX_ND * 17], lds_ws[2 * SB_MAX_ND * RES_GRP];
    __shared__ int gave_up;
    __shared__ cplx sbeta[NDT], scp[NDT];
    // the scalar stage's operands, fetched behind the apply (below): the |r|^2 partials' wave sums (+ the value that needs no
    // fold), and den[0..NDT) | CLOSE: lc->cx[0..NDT) | CLOSE: column m of the coefficient table, the entries lean_close_coef reads
    __shared__ double lds_rr[17];
    __shared__ cplx sstg[SB_STAGE_N];
    extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];   // Ar of this workgroup's rows: [trip][thread]
    if (a.st->stop_at < a.st->base + a.it) return;
    const int lb = logical_workgroup(a.rm, (int)blockIdx.x, (int)gridDim.x);
    if (lb >= a.nlogical) return;
    cplx *arL = reinterpret_cast<cplx *>(sb_smem);
    const int tid = (int)threadIdx.x;
    ResSync sy;
    res_sync_init(sy, a.slots, a.gen0, a.nlogical, lb, a.abort_dev, a.spin_limit, lds_pw, lds_ws, &gave_up);
    if (a.test_stall && lb == a.test_stall - 1) return;
    int64_t i0, end, stride;
    row_range(a.rm, lb, a.nlogical, a.n, &i0, &end, &stride);
    auto row = [&](int t) -> int64_t { return i0 + (int64_t)t * stride; };
    // the rows' byte offsets (n < 2^28 rows here), one VGPR per trip for every stream: the loads and stores take a scalar base
    // and this offset (64-bit addresses per stream and trip would be kept from pass 1 to the build, and spill)
    // (POL::OTF: only trip 0's offset is held; the others are formed where they are used, from the row step in a scalar register)
    uint32_t off[OTF ? 1 : SB_MAX_TRIPS];
#pragma unroll
    for (int t = 0; t < (OTF ? 1 : SB_MAX_TRIPS); t++) off[t] = (uint32_t)row(t) * (uint32_t)sizeof(cplx);
    const uint32_t soff = OTF ? (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)stride * (uint32_t)sizeof(cplx))) : 0u;
    auto at = [&](auto *p, int t) {
        if constexpr (OTF) return sb_elem(p, off[0] + (uint32_t)t * soff);
        else return sb_elem(p, off[t]);
    };
    cplx rk[SB_MAX_TRIPS];   // r of the thread's rows, from the apply to the last pass
    // ---- apply (gcr_fused.hip step_apply_kernel): Ar to LDS, r kept ----
#pragma unroll
    for (int t = 0; t < SB_MAX_TRIPS; t++) {
        const int64_t i = row(t);
        rk[t] = make_double2(0., 0.);
        // (the stencil's columns are clamped to 0..n-1: 32-bit byte offsets from the scalar base, as below)
        const auto xj = [&](int32_t j) -> cplx { return *sb_elem(a.x, (uint32_t)j * (uint32_t)sizeof(cplx)); };
        if constexpr (POL::OWN) {
            // The row product hands the row's own r back (the stencil's diagonal slot: the host has checked that it is one,
            // sten_lane_middle) and, with POL::LANES, takes r[i - 1] and r[i + 1] from the neighbouring lanes: a whole wave enters,
            // also its lanes beyond `end` (a wave's rows are 64 consecutive ones from a multiple of 64: its first lane decides)
            static_assert(REALC, "the forms for complex coefficients spill with it");
            if (__builtin_amdgcn_readfirstlane((int32_t)i) < (int32_t)end) {
                cplx own;
                const cplx sum = sten_row_product_own_t<1, POL::LANES>(a.m, i, xj, own);
                if (i < end) {
                    rk[t] = own;
                    arL[t * RED_THREADS + tid] = a.m.shift ? csub(own, cmul(a.m.k, sum)) : sum;
                }
            }
        } else if (i < end) {
            const PatLds pl{nullptr, nullptr, nullptr};
            cplx sum;
            if constexpr (REALC) sum = sten_row_product_t<7, false, 1>(a.m, i, xj);
            else sum = fused_row_product<3, 7>(a.m, i, 0, pl, xj);
            rk[t] = *at(a.x, t);
            arL[t * RED_THREADS + tid] = a.m.shift ? csub(rk[t], cmul(a.m.k, sum)) : sum;
        }
        __builtin_amdgcn_sched_barrier(0);   // (one trip's gathers in registers at a time)
    }
    // ---- <Ar, Ap_j>, one direction (all trips) at a time: its two sums go through the wave trees as soon as they are final ----
    // The directions are walked LAST TO FIRST (every direction's pair of sums has its own LDS slots, so their order enters no
    // sum): Ap_0 comes last and its first KT rows stay in registers for the build, which starts with Ap_0 — those rows are not
    // read again (the streams are non-temporal and a vector is an XCD's whole L2: a re-read is a trip to memory).  POL::TAIL: the
    // rows of Ap_0 that are not kept (<= 1 MB per XCD each) are loaded temporally, for the build's re-read to hit that L2.
    cplx pre[KT > 0 ? KT : 1];
    // The scalar stage behind exchange 1 needs, besides the exchanged sums, only values that were in memory when the launch began:
    // the |r|^2 partials and den[] (written behind poll 2 of the launch before, or by the kernels before), bnorm2 and tol2 (the
    // solve's start), and at the close lc->cx, lc->t and lc->T (poll 2 of the launch before, lean_table_row of earlier launches).
    // Loaded behind that exchange they are three dependent round trips to memory at the one moment when the whole grid has no
    // load in flight.  Here they are requested behind the apply, in one round trip while the workgroup's other waves still
    // stream, and parked in LDS — the |r|^2 partials as fold_partials' wave sums — so that behind the poll only LDS reads, the
    // divisions and the coefficient arithmetic are left.  (Held in registers over pass 1's first direction and parked behind it,
    // or requested ahead of the apply, the close at 5 directions and two forms for complex coefficients need scratch.)
    // Reads only: every write of the stage stays behind the poll (other workgroups may still be in their prologue), and lc->cx
    // and den[], which workgroup 0 rewrites behind poll 2, are read before this workgroup publishes exchange 2, as before.  No
    // vector register lives across a poll for it.  The last wave fetches den / cx / the table: the first waves hold the
    // exchange's hop-1 tasks.
    const bool folds = XR || lb == 0;
    double stg_r = 0.;
    cplx stg_c = make_double2(0., 0.);
    const int stg_i = tid - (RED_THREADS - 64);
    if (folds) stg_r = a.nblkR == 1 ? (tid == 0 ? a.partsR[0] + 0. : 0.) : (tid < a.nblkR ? a.partsR[tid] : 0.);
    if (stg_i >= 0 && stg_i < SB_STAGE_N) stg_c = *sb_stage_src<NDT>(a.den, a.lc, stg_i);
    if (folds) sb_stage_rr_waves(stg_r, a.nblkR, lds_rr);
    if (stg_i >= 0 && stg_i < SB_STAGE_N) sstg[stg_i] = stg_c;
    __builtin_amdgcn_sched_barrier(0);
    {
#pragma unroll
        for (int jj = 0; jj < NDT; jj++) {
            const int j = NDT - 1 - jj;
            cplx b[SB_MAX_TRIPS];
#pragma unroll
            for (int t = 0; t < SB_MAX_TRIPS; t++) {
                if (POL::TAIL && j == 0 && t >= KT) b[t] = row(t) < end ? ld_stream<false>(at(a.aps[j], t)) : make_double2(0., 0.);
                else b[t] = row(t) < end ? ld_stream<true>(at(a.aps[j], t)) : make_double2(0., 0.);
            }
            double v[2] = {0., 0.};
#pragma unroll
            for (int t = 0; t < SB_MAX_TRIPS; t++) {
                if (row(t) < end) {
                    const cplx tt = cconj_mul(arL[t * RED_THREADS + tid], b[t]);
                    v[0] += tt.x;
                    v[1] += tt.y;
                }
            }
            if constexpr (KT > 0) {
                if (j == 0) {
#pragma unroll
                    for (int u = 0; u < KT; u++) pre[u] = b[u];
                }
            }
            sb_wave_pair_to_lds(v, lds, 2 * j);
            __builtin_amdgcn_sched_barrier(0);
        }
        const double mine = sb_block_owner_from_lds<2 * NDT>(lds);
        if (tid < 2 * NDT) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((1 * RES_NV + tid) * RES_BLK + lb) * 16, 0, RES_SC1);
        }
    }
    // the stop decision, ahead of the poll as well (the barrier above has made lds_rr visible); in a scalar register from here on
    bool ends_here = false;
    if (folds) ends_here = __builtin_amdgcn_readfirstlane(!((sb_stage_rr(a.nblkR, lds_rr) / a.st->bnorm2) > a.st->tol2)) != 0;
    if (!res_collect<2 * NDT>(sy, 1)) {
        res_abort(a.abort_dev, a.abort_host);
        for (int64_t i = i0; i < end; i += stride) a.ap_out[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
        if (tid < 4) a.partsA[tid * RED_MAX_BLOCKS + lb] = __builtin_nan("");
        return;
    }
    // ---- direction build (as in step_build_kernel) ----
    // (the scalar stage's operands are in LDS, its |r|^2 fold and stop decision made: see pass 1; the writes are here)
    if (lb == 0 && tid == 0) {
        close_step(a.st, a.it, sb_stage_rr(a.nblkR, lds_rr), a.hist, a.hist_cap, CLOSE);
        if (CLOSE) a.st->closed = 1;
    }
    if (tid < NDT) sbeta[tid] = cdiv(make_double2(res_total(sy, 2 * tid), res_total(sy, 2 * tid + 1)), sstg[tid]);
    __syncthreads();
    if constexpr (CLOSE) {
        if (tid < NDT) scp[tid] = sb_stage_close_coef<NDT>(sstg + 2 * NDT + tid * NDT, sbeta, tid);
        __syncthreads();
    }
    if (!CLOSE && lb == 0 && tid <= NDT) lean_table_row<NDT>(a.lc, sbeta, tid);
    {
        cplx beta[NDT];   // (in scalar registers once: read from LDS per batch, the compiler keeps them in vector registers)
#pragma unroll
        for (int j = 0; j < NDT; j++) beta[j] = to_sgpr(sbeta[j]);
        double v[4] = {0., 0., 0., 0.};
#pragma unroll
        for (int t0 = 0; t0 < SB_MAX_TRIPS; t0 += TB) {
            cplx ac[TB];
#pragma unroll
            for (int u = 0; u < TB; u++) ac[u] = make_double2(0., 0.);
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx aj[TB];
#pragma unroll
                for (int u = 0; u < TB; u++)
                    aj[u] = (j == 0 && t0 + u < KT) ? pre[t0 + u < KT ? t0 + u : 0]
                            : row(t0 + u) < end   ? ld_stream<NTS>(at(a.aps[j], t0 + u))
                                                  : make_double2(0., 0.);
#pragma unroll
                for (int u = 0; u < TB; u++) ac[u] = csub(ac[u], cmul(beta[j], aj[u]));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int u = 0; u < TB; u++) {
                const int t = t0 + u;
                const int64_t i = row(t);
                if (i < end) {
                    const cplx an = cadd(arL[t * RED_THREADS + tid], ac[u]);
                    *at(a.ap_out, t) = an;
                    if (XR) arL[t * RED_THREADS + tid] = an;   // (A r is not needed any more; the update below wants Ap')
                    const cplx tt = cconj_mul(rk[t], an);
                    v[0] += tt.x; v[1] += tt.y;
                    const cplx w = cconj_mul(an, an);
                    v[2] += w.x; v[3] += w.y;
                }
            }
        }
        const double mine = block_sum_owner<4>(v, lds);
        if (tid < 4) a.partsA[tid * RED_MAX_BLOCKS + lb] = mine;
        if (XR && tid < 4) {
            const v4i w4 = {__double2loint(mine), __double2hiint(mine), (int)sy.gen, 0};
            __builtin_amdgcn_raw_buffer_store_b128(w4, sy.slots, ((2 * RES_NV + tid) * RES_BLK + lb) * 16, 0, RES_SC1);
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
        for (int t0 = 0; t0 < SB_MAX_TRIPS; t0 += TB) {
            cplx xv[TB], pc[TB];
#pragma unroll
            for (int u = 0; u < TB; u++) {
                xv[u] = row(t0 + u) < end ? *at(a.xvec, t0 + u) : make_double2(0., 0.);
                pc[u] = make_double2(0., 0.);
            }
#pragma unroll
            for (int j = 0; j < NDT; j++) {
                cplx pj[TB];
#pragma unroll
                for (int u = 0; u < TB; u++) pj[u] = row(t0 + u) < end ? ld_stream<NTS>(at(a.ps[j], t0 + u)) : make_double2(0., 0.);
#pragma unroll
                for (int u = 0; u < TB; u++) {
                    xv[u] = cadd(xv[u], cmul(cx[j], pj[u]));
                    pc[u] = csub(pc[u], cmul(cp[j], pj[u]));
                }
            }
#pragma unroll
            for (int u = 0; u < TB; u++) {
                const int64_t i = row(t0 + u);
                if (i < end) {
                    *at(a.xvec, t0 + u) = xv[u];
                    st_stream<NTS>(at(a.p_out, t0 + u), cadd(rk[t0 + u], pc[u]));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (XR) {
        if (!res_collect<4>(sy, 2)) {
            res_abort(a.abort_dev, a.abort_host);
            for (int64_t i = i0; i < end; i += stride) a.xr_out[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
            if (threadIdx.x == 0) a.partsR_out[lb] = __builtin_nan("");
            return;
        }
        if (ends_here) return;
        const cplx alpha = sb_xr_alpha(sy, a.st, a.lc, a.xr_den_slot, a.xr_slot, lb);
        double vr[1] = {0.};
#pragma unroll
        for (int t = 0; t < SB_MAX_TRIPS; t++) {
            const int64_t i = row(t);
            if (i < end) {
                const cplx rn = csub(rk[t], cmul(alpha, arL[t * RED_THREADS + tid]));
                *at(a.xr_out, t) = rn;
                vr[0] += rn.x * rn.x + rn.y * rn.y;
            }
        }
        const double tot = block_sum_owner<1>(vr, lds);
        if (threadIdx.x == 0) a.partsR_out[lb] = tot;
    }
