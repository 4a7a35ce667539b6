// Sparse operators on the device, the apply half: Sparse<long> (stencil view / row-pattern dictionary / ELL slab + CSR tail) and
// HierarchicalSparse<long,int> (block-CSR of dense blocks).  spmv_build.hip constructs the formats.
//
//   reference: Sparse::operator()            src/Operator.h:330-346
//              DiracOp::operator()           src/Operator.h:569-575   (fused epilogue y = x - k*sum)
//              HierarchicalSparse::operator()  src/HierarchicalSparse.h:101-161
//              Dense::operator()             src/Operator.h:159-173
//
// All of it is HBM-bound (8 flop per 20 stored bytes): the kernels are built around coalesced
// 16-B-per-lane streams of the matrix, L2/MALL-served gathers of x, and wave64 shuffle / LDS
// reductions.  No MFMA.
#include "internal.h"
#include "reduce.h"
#include "spmv_dev.h"

namespace mgcr {

bool csr_stencil_active(const CsrDev &A) { return A.sten_ns > 0 && stencil_enabled(); }

// has the solve this apply belongs to stopped on the device?  (skip = {stop_at, base}, gcr.hip DevState; null: stand-alone apply.)
// Read through the constant address space: scalar loads wherever the call stands.
__device__ __forceinline__ bool stop_flag(const int *skip, int skip_it) {
    typedef const int __attribute__((address_space(4))) *stop_ptr;
    const stop_ptr sk = (stop_ptr)(uintptr_t)skip;
    return skip && sk[0] < sk[1] + skip_it;
}

template <int WT, bool SHIFT, bool XCD, bool REALV, bool NT>
__global__ void __launch_bounds__(256) ell_spmv_rowthread(int64_t row_begin, int64_t row_count, int64_t npad, int32_t Wrt,
                                                          int64_t ntiles, const void *__restrict__ val,
                                                          const int32_t *__restrict__ col, const cplx *__restrict__ x,
                                                          const cplx *__restrict__ xh, int32_t n_own,
                                                          cplx *__restrict__ y, cplx k, const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it) {
    // One scalar batch for every argument (pinned by the empty asm) instead of one dependent fetch per early exit: a wave
    // lives a few microseconds and each dependent scalar round trip in front of its first load costs ~0.2 us of that.  The
    // solver's stop flag (skip = {stop_at, base}: see gcr.hip DevState) is looked at while the loads fly and only gates the store.
    asm volatile("" ::"s"(row_begin), "s"(row_count), "s"(npad), "s"(Wrt), "s"(ntiles), "s"(val), "s"(col), "s"(x), "s"(xh), "s"(n_own), "s"(y),
                 "s"(w), "s"(skip), "s"(skip_it));
    int64_t tile = XCD ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    int64_t rloc = tile * 256 + threadIdx.x;
    if (rloc >= row_count) return;
    int64_t row = row_begin + rloc;
    const int32_t W = WT ? WT : Wrt;
    cplx sum = make_double2(0., 0.);
    bool stopped = false;
    if (WT) {
        int32_t j[WT ? WT : 1];
        cplx xv[WT ? WT : 1];
#pragma unroll
        for (int32_t c = 0; c < W; c++) j[c] = ldcol<NT>(col + (int64_t)c * npad + row);
        stopped = stop_flag(skip, skip_it);
#pragma unroll
        for (int32_t c = 0; c < W; c++) xv[c] = gather_x(x, xh, n_own, j[c]);
#pragma unroll
        for (int32_t c = 0; c < W; c++) sum = cadd(sum, vmul<REALV, NT>(val, (int64_t)c * npad + row, xv[c]));
    } else {
        stopped = stop_flag(skip, skip_it);
#pragma unroll 4
        for (int32_t c = 0; c < W; c++) {
            int32_t j = ldcol<NT>(col + (int64_t)c * npad + row);
            sum = cadd(sum, vmul<REALV, NT>(val, (int64_t)c * npad + row, gather_x(x, xh, n_own, j)));
        }
    }
    if (!stopped) y[row] = SHIFT ? csub((w ? w : x)[row], cmul(k, sum)) : sum;
}

// ELL slab, one thread per row, x window in LDS (banded irregular matrices: CsrDev::win_h).  A workgroup owns 1024 consecutive
// rows; x[r0 - H, r0 + 1024 + H) is read once, coalesced, into LDS and every column inside it is served from there — the few
// outside take the global gather.  Same products, added in the same (CSR) order as ell_spmv_rowthread: same bits.
// TAIL: the CSR tail of the tile's rows in the SAME launch.  The tail entries of consecutive rows are one contiguous piece of the
// tail arrays: the workgroup streams it 1024 entries at a time (coalesced), gathers x from the window it already holds, stages the
// products in LDS, and every thread adds the products of ITS row in CSR order onto a tail sum; y = (ELL sum) + (tail sum) is
// written once — csr_tail_chunk_kernel's arithmetic and order (same bits) without the second launch, the second gather of x from
// memory and the read-modify-write of y.  Rows whose tail is longer than a chunk (TAIL_CAP) are left to csr_tail_kernel.
constexpr int WIN_TAIL_PER = 2;                           // tail entries per thread and trip
constexpr int WIN_TAIL_CH = WIN_TAIL_PER * ELL_WIN_ROWS;   // tail entries staged per trip (32 KB of products)
template <bool SHIFT, bool REALV, int H, bool TAIL>
__global__ void __launch_bounds__(ELL_WIN_ROWS) ell_spmv_window(int64_t nrow, int64_t npad, int32_t W, int64_t ntiles, const void *__restrict__ val,
                                                                const int32_t *__restrict__ col, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                                cplx k, const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it,
                                                                const int32_t *__restrict__ tile_tail, const int32_t *__restrict__ row_tail,
                                                                const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                                const cplx *__restrict__ tail_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char win_smem[];
    cplx *win = reinterpret_cast<cplx *>(win_smem);
    constexpr int WLEN = ELL_WIN_ROWS + 2 * H;
    cplx *prod = win + WLEN;   // [WIN_TAIL_CH] (TAIL only)
    const int64_t tile = ntiles >= 64 ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    const int64_t r0 = tile * ELL_WIN_ROWS, base = r0 - H;
    const int64_t row = r0 + threadIdx.x;
    const bool live = row < nrow;
    // the row's first columns are requested together with the window (they do not depend on it)
    int32_t j0 = 0, j1 = 0;
    if (live) {
        j0 = ldcol<true>(col + row);
        if (W > 1) j1 = ldcol<true>(col + npad + row);
    }
    int32_t t0 = 0, t1 = 0, ti = -1;
    if (TAIL) {
        t0 = tile_tail[tile];
        t1 = tile_tail[tile + 1];
        if (live) ti = row_tail[row];
    }
    for (int t = threadIdx.x; t < WLEN; t += ELL_WIN_ROWS) {
        int64_t g = base + t;
        g = g < 0 ? 0 : g >= nrow ? nrow - 1 : g;
        win[t] = x[g];
    }
    const bool stopped = stop_flag(skip, skip_it);
    __syncthreads();
    if (stopped) return;   // (uniform)
    auto xat = [&](int32_t j) -> cplx {
        const int64_t off = (int64_t)j - base;
        return (off >= 0 && off < WLEN) ? win[off] : x[j];
    };
    cplx sum = make_double2(0., 0.);
    if (live) {
        sum = cadd(sum, vmul<REALV, true>(val, row, xat(j0)));
        if (W > 1) sum = cadd(sum, vmul<REALV, true>(val, npad + row, xat(j1)));
#pragma unroll 4
        for (int32_t c = 2; c < W; c++) {
            const int32_t j = ldcol<true>(col + (int64_t)c * npad + row);
            sum = cadd(sum, vmul<REALV, true>(val, (int64_t)c * npad + row, xat(j)));
        }
    }
    if (!TAIL) {
        if (live) y[row] = SHIFT ? csub((w ? w : x)[row], cmul(k, sum)) : sum;
        return;
    }
    const int32_t e0 = tail_ptr[t0], e1 = tail_ptr[t1];
    int32_t rb = 0, re = 0;
    if (ti >= 0) { rb = tail_ptr[ti]; re = tail_ptr[ti + 1]; }
    cplx tsum = make_double2(0., 0.);
    // the next trip's columns and values are requested before this trip's products are formed and summed: their latency hides
    // behind the LDS phase (two workgroups per CU do not hide it by themselves)
    int32_t jn[WIN_TAIL_PER];
    cplx vn[WIN_TAIL_PER];
    auto fetch = [&](int32_t cb) {
#pragma unroll
        for (int q = 0; q < WIN_TAIL_PER; q++) {
            const int32_t e = cb + q * ELL_WIN_ROWS + (int32_t)threadIdx.x;
            jn[q] = -1;
            vn[q] = make_double2(0., 0.);
            if (e < e1) {
                jn[q] = tail_col[e];
                vn[q] = make_double2(__builtin_nontemporal_load(&tail_val[e].x), __builtin_nontemporal_load(&tail_val[e].y));
            }
        }
    };
    if (e0 < e1) fetch(e0);
    for (int32_t cb = e0; cb < e1; cb += WIN_TAIL_CH) {   // uniform trip count
        int32_t jc[WIN_TAIL_PER];
        cplx vc[WIN_TAIL_PER];
#pragma unroll
        for (int q = 0; q < WIN_TAIL_PER; q++) { jc[q] = jn[q]; vc[q] = vn[q]; }
        if (cb + WIN_TAIL_CH < e1) fetch(cb + WIN_TAIL_CH);
#pragma unroll
        for (int q = 0; q < WIN_TAIL_PER; q++)
            if (jc[q] >= 0) prod[q * ELL_WIN_ROWS + threadIdx.x] = cmul(vc[q], xat(jc[q]));
        __syncthreads();
        const int32_t ib = (rb > cb ? rb : cb) - cb, ie = (re < cb + WIN_TAIL_CH ? re : cb + WIN_TAIL_CH) - cb;
        {   // this row's products of the trip, in CSR order (four independent LDS reads in flight)
            int32_t i = ib;
            for (; i + 4 <= ie; i += 4) {
                const cplx p0 = prod[i], p1 = prod[i + 1], p2 = prod[i + 2], p3 = prod[i + 3];
                tsum = cadd(cadd(cadd(cadd(tsum, p0), p1), p2), p3);
            }
            for (; i < ie; i++) tsum = cadd(tsum, prod[i]);
        }
        __syncthreads();
    }
    if (live) {
        if (SHIFT) {
            cplx v = csub((w ? w : x)[row], cmul(k, sum));
            if (ti >= 0) v = csub(v, cmul(k, tsum));
            y[row] = v;
        } else {
            y[row] = ti >= 0 ? cadd(sum, tsum) : sum;
        }
    }
}

// Row-pattern dictionary SpMV (L = 1): one thread per row; the row's 2-byte id selects the table row
// holding its W column offsets (and, MODE 1, its W values).  Interior rows of a wave share one id, so
// the table loads are single-line broadcasts out of L1.  Same multiply/add order as ell_spmv_rowthread.
template <int WT, bool SHIFT, bool XCD, int MODE, bool REALV>
__global__ void __launch_bounds__(256) pat_spmv_rowthread(int64_t row_begin, int64_t row_count, int64_t npad, int32_t Wrt,
                                                          int64_t ntiles, const uint16_t *__restrict__ pid,
                                                          const int32_t *__restrict__ poff, const double *__restrict__ pre,
                                                          const double *__restrict__ pim, const void *__restrict__ val,
                                                          const cplx *__restrict__ x, const cplx *__restrict__ xh, int32_t n_own,
                                                          cplx *__restrict__ y, cplx k, const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    int64_t tile = XCD ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    int64_t rloc = tile * 256 + threadIdx.x;
    if (rloc >= row_count) return;
    const int64_t row = row_begin + rloc;
    const int32_t W = WT ? WT : Wrt;
    const int32_t t0 = (int32_t)__builtin_nontemporal_load(pid + row) * W;
    cplx sum = make_double2(0., 0.);
    auto term = [&](int32_t c, cplx xv) -> cplx {
        if (MODE == 1) {
            if (REALV) {
                double v = pre[t0 + c];
                return make_double2(v * xv.x, v * xv.y);
            }
            return cmul(make_double2(pre[t0 + c], pim[t0 + c]), xv);
        }
        return vmul<REALV, true>(val, (int64_t)c * npad + row, xv);
    };
    if (WT) {
        cplx xv[WT ? WT : 1];
#pragma unroll
        for (int32_t c = 0; c < W; c++) xv[c] = gather_x(x, xh, n_own, (int32_t)row + poff[t0 + c]);
#pragma unroll
        for (int32_t c = 0; c < W; c++) sum = cadd(sum, term(c, xv[c]));
    } else {
#pragma unroll 4
        for (int32_t c = 0; c < W; c++) sum = cadd(sum, term(c, gather_x(x, xh, n_own, (int32_t)row + poff[t0 + c])));
    }
    y[row] = SHIFT ? csub((w ? w : x)[row], cmul(k, sum)) : sum;
}

// Same, with the pattern table staged in LDS (one dependent memory round trip less per row: id -> LDS ->
// gathers; 17.6 against 20.7 us at Poisson 128^3).  MODE 1 only.  R rows per thread with all id loads and
// gathers in flight together was measured too (R = 2, 4; 256 / 512 threads): no faster than R = 1, warm or
// cold; nor was staging the workgroup's own 256..1024 entries of x in LDS to serve the +-1 / +-n columns
// (26 against 25 us cold) — PMC: TA busy 61 %, L2 hit rate 0.61, 90 % of wave cycles waiting; the kernel
// moves 71 MB in 17 (warm) .. 25 us (cold caches) where a 67 MB copy takes 11.4 us.
template <int WT, bool SHIFT, bool REALV, int R, int BLK>
__global__ void __launch_bounds__(BLK) pat_spmv_lds(int64_t row_begin, int64_t row_count, int32_t Wrt, int64_t ntiles, int xcd,
                                                    int32_t npat, const uint16_t *__restrict__ pid,
                                                    const int32_t *__restrict__ poff, const double *__restrict__ pre,
                                                    const double *__restrict__ pim, const cplx *__restrict__ x,
                                                    const cplx *__restrict__ xh, int32_t n_own, cplx *__restrict__ y, cplx k,
                                                    const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pat_smem[];
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    const int64_t tile = xcd ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    const int32_t W = WT ? WT : Wrt;
    const int32_t ne = npat * W;
    double *sre = reinterpret_cast<double *>(pat_smem);
    double *sim = sre + (REALV ? 0 : ne);
    int32_t *soff = reinterpret_cast<int32_t *>(sim + ne);
    int64_t row[R];
    bool live[R];
    int32_t t0[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t rloc = tile * (BLK * R) + r * BLK + threadIdx.x;
        live[r] = rloc < row_count;
        row[r] = row_begin + (live[r] ? rloc : 0);
        t0[r] = (int32_t)__builtin_nontemporal_load(pid + row[r]) * W;
    }
    for (int32_t e = threadIdx.x; e < ne; e += BLK) {
        soff[e] = poff[e];
        sre[e] = pre[e];
        if (!REALV) sim[e] = pim[e];
    }
    __syncthreads();
    if (WT) {
        cplx xv[R][WT ? WT : 1];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int32_t c = 0; c < W; c++) xv[r][c] = gather_x(x, xh, n_own, (int32_t)row[r] + soff[t0[r] + c]);
#pragma unroll
        for (int r = 0; r < R; r++) {
            cplx sum = make_double2(0., 0.);
#pragma unroll
            for (int32_t c = 0; c < W; c++) {
                cplx t;
                if (REALV) { double v = sre[t0[r] + c]; t = make_double2(v * xv[r][c].x, v * xv[r][c].y); }
                else t = cmul(make_double2(sre[t0[r] + c], sim[t0[r] + c]), xv[r][c]);
                sum = cadd(sum, t);
            }
            if (live[r]) y[row[r]] = SHIFT ? csub((w ? w : x)[row[r]], cmul(k, sum)) : sum;
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; r++) {
            cplx sum = make_double2(0., 0.);
#pragma unroll 4
            for (int32_t c = 0; c < W; c++) {
                cplx xv = gather_x(x, xh, n_own, (int32_t)row[r] + soff[t0[r] + c]);
                cplx t;
                if (REALV) { double v = sre[t0[r] + c]; t = make_double2(v * xv.x, v * xv.y); }
                else t = cmul(make_double2(sre[t0[r] + c], sim[t0[r] + c]), xv);
                sum = cadd(sum, t);
            }
            if (live[r]) y[row[r]] = SHIFT ? csub((w ? w : x)[row[r]], cmul(k, sum)) : sum;
        }
    }
}

// Stencil view SpMV (MODE 3, spmv_dev.h sten_row_product): BLK consecutive rows per workgroup, waves aligned to
// multiples of 64 rows (`first` = row_begin rounded down), one memory round trip per row.
template <int NS, bool RARE, bool SHIFT, int BLK>
__global__ void __launch_bounds__(BLK) sten_spmv(RowMat m, int64_t row_begin, int64_t row_end, int64_t first, int64_t ntiles, int xcd,
                                                 const cplx *__restrict__ x, cplx *__restrict__ y, const cplx *__restrict__ w,
                                                 const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    const int64_t tile = xcd ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    const int64_t rloc = first + tile * BLK + threadIdx.x;
    if ((rloc | 63) < row_begin || (rloc & ~(int64_t)63) >= row_end) return;   // the whole wave lies outside
    const bool live = rloc >= row_begin && rloc < row_end;
    const cplx sum = sten_row_product<NS, RARE>(m, rloc, [&](int32_t j) -> cplx { return gather_x(x, m.xh, m.n_own, j); });
    if (live) y[rloc] = SHIFT ? csub((w ? w : x)[rloc], cmul(m.k, sum)) : sum;
}

// The same with an LDS window: the workgroup's BLK entries of x plus sten_halo entries on either side are staged once
// (one coalesced load per thread, the halo by the first 2 * sten_halo threads) and the slots close to the diagonal
// (sten_near: +-1, +-n of a grid) are read from there; the far slots (+-n^2) are requested before the barrier.  A
// 7-point row then costs ~3.5 loads through L1 / L2 instead of 7 — tools/spmv_lab.hip on MI355X, Poisson 256^3: 130
// against 151 us with cold caches (the +-n neighbours, which the neighbouring workgroups fetch at the same time, are
// the expensive ones), 128^3: 20.4 against 21.9 us.  Same slot order, same selects: same bits.  NEAR is a template
// parameter (the kernel exists for the mask of a 3-D stencil, slots 1..5 of 7): with a run-time mask the compiler keeps
// the gathered values in scratch memory and waits for every load in turn — 4x slower than no window at all.
template <int NS, bool RARE, bool SHIFT, int BLK, unsigned NEAR, bool DMA>
__global__ void __launch_bounds__(BLK) sten_spmv_tile(RowMat m, int64_t row_begin, int64_t row_end, int64_t first, int64_t ntiles, int xcd,
                                                      const cplx *__restrict__ x, cplx *__restrict__ y, const cplx *__restrict__ w,
                                                      const int *__restrict__ skip, int skip_it) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sten_smem[];
    constexpr int NC = RARE ? STEN_COMMON : NS;   // rare-tail layout: slots NC.. are looked at after the common sum
    // A wave of this kernel lives ~3 us and every DEPENDENT scalar fetch in front of its gathers costs ~0.2 us of that (measured:
    // one kernel argument fetched late = +6 % kernel time).  So: every argument the gathers need is fetched in ONE batch (the
    // empty asm pins them), the gathers go out, and only then come the scalar loads from memory — presence words, the solver's
    // stop flag (skip = {stop_at, base}, gcr.hip DevState), whose answers nobody needs before the window is filled.
    const int32_t H = m.sten_halo, last = m.sten_last, n_own = m.n_own, nwaves = m.sten_nwaves, pstride = m.sten_stride;
    const cplx *const xh = m.xh;
    const uint64_t *const planes = m.sten_planes;
    int32_t off[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) off[c] = m.sten_off[c];
    asm volatile("" ::"s"(H), "s"(last), "s"(n_own), "s"(nwaves), "s"(pstride), "s"(xh), "s"(planes), "s"(x), "s"(first), "s"(ntiles), "s"(xcd),
                 "s"(row_begin), "s"(row_end), "s"(skip), "s"(skip_it), "s"(y));
    const int realv = m.realv;
    double re[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        re[c] = m.sten_re[c];
        asm volatile("" ::"s"(off[c]), "s"(re[c]));
    }
    asm volatile("" ::"s"(realv));
    const int64_t tile = xcd ? xcd_tile(ntiles) : (int64_t)blockIdx.x;
    if (tile >= ntiles) return;
    cplx *sx = reinterpret_cast<cplx *>(sten_smem);   // [H + BLK + H], entry e = column base - H + e
    const int64_t base = first + tile * BLK;
    const int64_t rloc = base + threadIdx.x;
    const bool live = rloc >= row_begin && rloc < row_end;
    auto clampj = [&](int64_t j) -> int32_t { return (int32_t)(j < 0 ? 0 : j > last ? last : j); };
    cplx xv[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        xv[c] = make_double2(0., 0.);
        if (!(NEAR >> c & 1u)) xv[c] = gather_x(x, xh, n_own, clampj(rloc + off[c]));
    }
    cplx own = make_double2(0., 0.), halo = make_double2(0., 0.);
    int hidx = -1;
    if constexpr (DMA) {
        // the window is filled by the memory system itself (gfx950 global_load_lds_dwordx4: 16 bytes per lane, a wave's 64 entries
        // land contiguously at the LDS address in M0): no registers, no ds_write between the data's arrival and the barrier —
        // 14.6-15.0 -> 14.3 us back to back at 128^3, 127-128 -> 122-123 us at 256^3 (cold: 22.0-22.6 -> 21.4, 131-132 -> 125-127).
        // (H is a multiple of 64 here: a wave of halo threads lies entirely left or entirely right of the tile.  The same fill in
        // the solver's windowed step kernels, gcr_fused.hip, LOSES 2 %: they need the row's own entry in registers afterwards
        // and the per-lane addresses cost what the data registers saved — measured, not kept.)
        const int wv = (int)(threadIdx.x >> 6) * 64;
        const int32_t jo = clampj(rloc);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(jo < n_own ? x + jo : xh + (jo - n_own)),
                                         (__attribute__((address_space(3))) void *)(sx + H + wv), 16, 0, 0);
        if ((int)threadIdx.x < 2 * H) {
            const int t = (int)threadIdx.x;
            const int32_t jh = clampj(t < H ? base - H + t : base + BLK + (t - H));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(jh < n_own ? x + jh : xh + (jh - n_own)),
                                             (__attribute__((address_space(3))) void *)(sx + (t < H ? 0 : BLK) + wv), 16, 0, 0);
        }
    } else {
        own = gather_x(x, xh, n_own, clampj(rloc));
        if ((int)threadIdx.x < 2 * H) {
            const int t = (int)threadIdx.x;
            halo = gather_x(x, xh, n_own, clampj(t < H ? base - H + t : base + BLK + (t - H)));
            hidx = t < H ? t : BLK + t;
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // every gather is in flight before anything else is asked for
    // presence words of this wave (rows beyond the padded end of the matrix have none: the planes array ends with a zero row)
    int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)(rloc >> 6));
    wave = wave < nwaves ? wave : nwaves;
    const sten_planes_ptr pp = (sten_planes_ptr)(uintptr_t)(planes + (int64_t)wave * pstride);
    uint64_t pl[NS];
#pragma unroll
    for (int c = 0; c < NS; c++) pl[c] = pp[c];
    const bool stopped = stop_flag(skip, skip_it);
    __builtin_amdgcn_sched_barrier(0);   // every load is in flight before the first one is waited for
    if constexpr (DMA) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of the window has landed
    } else {
        sx[H + threadIdx.x] = own;
        if (hidx >= 0) sx[hidx] = halo;
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63);
    cplx sum = make_double2(0., 0.);
    if constexpr (RARE) sum = sten_pre_sum<-1>(m, rloc, pl[NC], lane, [&](int32_t j) -> cplx { return gather_x(x, xh, n_own, j); });
    // (the real / complex decision once, not per slot: per slot it put a scalar fetch and a branch between every two terms)
    if (realv) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            // a window entry outside the matrix is a clamped copy: only read by rows whose presence bit for the slot is clear
            const cplx v = (NEAR >> c & 1u) ? sx[H + (int)threadIdx.x + off[c]] : xv[c];
            const bool on = (pl[c] >> lane & 1ull) != 0ull;
            const cplx nsum = cadd(sum, make_double2(re[c] * v.x, re[c] * v.y));
            sum.x = on ? nsum.x : sum.x;
            sum.y = on ? nsum.y : sum.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const cplx v = (NEAR >> c & 1u) ? sx[H + (int)threadIdx.x + off[c]] : xv[c];
            const bool on = (pl[c] >> lane & 1ull) != 0ull;
            const cplx nsum = cadd(sum, cmul(make_double2(re[c], m.sten_im[c]), v));
            sum.x = on ? nsum.x : sum.x;
            sum.y = on ? nsum.y : sum.y;
        }
    }
    if (RARE) {
#pragma unroll
        for (int c = NC; c < NS; c++)
            if (pl[c] != 0ull && !(c == NC && m.sten_pre)) {   // wave-uniform: a wave of a boundary plane
                const cplx xr = gather_x(x, xh, n_own, clampj(rloc + m.sten_off[c]));
                const bool on = (pl[c] >> lane & 1ull) != 0ull;
                const cplx t = m.realv ? make_double2(m.sten_re[c] * xr.x, m.sten_re[c] * xr.y) : cmul(make_double2(m.sten_re[c], m.sten_im[c]), xr);
                const cplx nsum = cadd(sum, t);
                sum.x = on ? nsum.x : sum.x;
                sum.y = on ? nsum.y : sum.y;
            }
    }
    if (live && !stopped) y[rloc] = SHIFT ? csub((w ? w : x)[rloc], cmul(m.k, sum)) : sum;
}

// L in {2,4,8,16}: L consecutive lanes share a row; per chunk the (row, lane) pairs are contiguous
template <int L, bool SHIFT, bool REALV>
__global__ void __launch_bounds__(256) ell_spmv_lanes(int64_t row_begin, int64_t row_count, int64_t npad, int32_t nchunk,
                                                      const void *__restrict__ val, const int32_t *__restrict__ col,
                                                      const cplx *__restrict__ x, const cplx *__restrict__ xh, int32_t n_own,
                                                      cplx *__restrict__ y, cplx k, const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t rloc = t / L;
    int64_t row = row_begin + rloc;
    int64_t nrow = row_begin + row_count;
    int l = (int)(t % L);
    cplx sum = make_double2(0., 0.);
    if (row < nrow) {
#pragma unroll 4
        for (int32_t c = 0; c < nchunk; c++) {
            int64_t idx = ((int64_t)c * npad + row) * L + l;
            sum = cadd(sum, vmul<REALV>(val, idx, gather_x(x, xh, n_own, col[idx])));
        }
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        sum.x += __shfl_down(sum.x, off, L);
        sum.y += __shfl_down(sum.y, off, L);
    }
    if (row < nrow && l == 0) y[row] = SHIFT ? csub((w ? w : x)[row], cmul(k, sum)) : sum;
}

// CSR tail, rows longer than a chunk on their own (> TAIL_CAP entries): one wave per row, lanes stride the entries, wave64 tree
template <bool SHIFT>
__global__ void __launch_bounds__(256) csr_tail_kernel(int64_t n_long, const int32_t *__restrict__ tail_long, const int32_t *__restrict__ tail_rows,
                                                       const int32_t *__restrict__ tail_ptr,
                                                       const int32_t *__restrict__ tail_col,
                                                       const cplx *__restrict__ tail_val, const cplx *__restrict__ x,
                                                       const cplx *__restrict__ xh, int32_t n_own,
                                                       cplx *__restrict__ y, cplx k, const cplx *__restrict__ w, const int *__restrict__ skip, int skip_it) {
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (wave >= n_long) return;
    const int32_t t = tail_long[wave];
    int32_t beg = tail_ptr[t], end = tail_ptr[t + 1];
    cplx sum = make_double2(0., 0.);
    for (int32_t i = beg + lane; i < end; i += 64) sum = cadd(sum, cmul(tail_val[i], gather_x(x, xh, n_own, tail_col[i])));
    sum.x = wave_sum(sum.x);
    sum.y = wave_sum(sum.y);
    if (lane == 0) {
        int32_t row = tail_rows[t];
        y[row] = SHIFT ? csub(y[row], cmul(k, sum)) : cadd(y[row], sum);
    }
}

// CSR tail, everything else: one workgroup per CHUNK — a run of consecutive tail rows with at most TAIL_CAP entries and
// TAIL_THREADS rows (dealt at build time, spmv_layout.h deal_tail).  The chunk's entries are one contiguous piece of the tail
// arrays: all threads stream it with coalesced loads (4 entries per thread in flight: columns, values, the gathers of x),
// the products val * x are staged in LDS, and thread t then adds row t's products in CSR order — the reference's order
// (src/Operator.h:338-341) — onto the row's ELL sum.  Against one wave per row (rows of 1..55 entries: 1.7 M waves that each
// fetch half-used lines and spend their life in three dependent memory round trips) this streams whole lines once and keeps
// 32 waves per CU busy: 8 M-row skewed matrix (bench.py irregular_spmv), tail part: 0.69 ms -> see DESIGN.md.
template <bool SHIFT>
__global__ void __launch_bounds__(TAIL_THREADS) csr_tail_chunk_kernel(const int4 *__restrict__ chunks,
                                                                      const int32_t *__restrict__ tail_rows, const int32_t *__restrict__ tail_ptr,
                                                                      const int32_t *__restrict__ tail_col, const cplx *__restrict__ tail_val,
                                                                      const cplx *__restrict__ x, const cplx *__restrict__ xh, int32_t n_own,
                                                                      cplx *__restrict__ y, cplx k, const int *__restrict__ skip, int skip_it) {
    __shared__ cplx prod[TAIL_CAP];
    if (skip && skip[0] < skip[1] + skip_it) return;
    const int t = threadIdx.x;
    const int4 ch = chunks[blockIdx.x];   // one record: the entry range does not wait for a second, dependent fetch
    const int32_t r0 = ch.x, r1 = ch.y, e0 = ch.z, e1 = ch.w;
    // this thread's row (phase 2): requested now, used after the barrier
    int32_t rb = 0, re = 0, row = 0;
    if (r0 + t < r1) { rb = tail_ptr[r0 + t]; re = tail_ptr[r0 + t + 1]; row = tail_rows[r0 + t]; }
    constexpr int PER = TAIL_CAP / TAIL_THREADS;
    int32_t j[PER];
    cplx v[PER], xv[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int32_t e = e0 + q * TAIL_THREADS + t;
        j[q] = e < e1 ? tail_col[e] : -1;
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int32_t e = e0 + q * TAIL_THREADS + t;
        v[q] = e < e1 ? make_double2(__builtin_nontemporal_load(&tail_val[e].x), __builtin_nontemporal_load(&tail_val[e].y)) : make_double2(0., 0.);
        xv[q] = j[q] >= 0 ? gather_x(x, xh, n_own, j[q]) : make_double2(0., 0.);
    }
#pragma unroll
    for (int q = 0; q < PER; q++) prod[q * TAIL_THREADS + t] = cmul(v[q], xv[q]);
    __syncthreads();
    if (r0 + t < r1) {
        const cplx y0 = y[row];     // (requested before the LDS walk)
        cplx sum = make_double2(0., 0.);
        int32_t i = rb - e0;
        const int32_t ie = re - e0;
        for (; i + 4 <= ie; i += 4) {   // four independent LDS reads in flight, added in CSR order
            const cplx p0 = prod[i], p1 = prod[i + 1], p2 = prod[i + 2], p3 = prod[i + 3];
            sum = cadd(cadd(cadd(cadd(sum, p0), p1), p2), p3);
        }
        for (; i < ie; i++) sum = cadd(sum, prod[i]);
        y[row] = SHIFT ? csub(y0, cmul(k, sum)) : cadd(y0, sum);
    }
}

// measurement aid (bench.py: the ELL part and the CSR tail of a hybrid matrix timed separately): 0 = the whole apply,
// 1 = only the ELL slab's kernel, 2 = only the tail kernel (which then adds to whatever y holds).  mgcr_set_option("spmv_part").
static int g_spmv_part = 0;
int set_spmv_part(int part) {
    const int prev = g_spmv_part;
    g_spmv_part = part < 0 || part > 2 ? 0 : part;
    return prev;
}

// does the window kernel of A also multiply the chunk-sized tails (one launch for slab + tail)?  Not while bench.py times the
// two parts apart (spmv_part), not for the row block of a distributed matrix (halo columns live outside x)
static EnvSwitch g_window_tail("MGCR_ELL_WINDOW_TAIL");
static bool window_fuses_tail(const CsrDev &A) {
    // (H = 4096: the window alone takes 144 KB — with the products' 32 KB there is no room, and with 16 KB it measured slower than two launches)
    return g_window_tail.on() && A.win_h == 1024 && A.win_tile_tail && A.win_row_tail && g_spmv_part == 0;
}

static SkipRef g_skip;  // consulted by apply kernels (set by the GCR driver around its operator applies)
void set_apply_skip(SkipRef s) { g_skip = s; }
SkipRef get_apply_skip() { return g_skip; }

// `rows` rows in tiles of `tile`: from 64 tiles on, the grid is padded to a multiple of 8 and every XCD takes one band (xcd_tile)
struct Tiles { int64_t ntiles; bool xcd; unsigned grid; };
static Tiles tiles_of(int64_t rows, int tile) {
    const int64_t ntiles = (rows + tile - 1) / tile;
    return Tiles{ntiles, ntiles >= 64, (unsigned)(ntiles >= 64 ? ((ntiles + 7) / 8) * 8 : ntiles)};
}
// rows [row_begin, row_begin + row_count) of the ELL part: y = A x, or (SHIFT) y = w - k A x
struct Rows { int64_t row_begin, row_count; const cplx *x, *xh; int32_t n_own; cplx *y; cplx k; const cplx *w; };
static const void *slab_values(const CsrDev &A) { return A.ell_val_re ? (const void *)A.ell_val_re : (const void *)A.ell_val; }
// (MGCR_SPMV_NT: on by default, +3 % GCR iterations/s at 128^3, measured; =0 turns it off)
static EnvSwitch g_sten_tile("MGCR_STENCIL_TILE"), g_sten_dma("MGCR_STENCIL_DMA"), g_spmv_nt("MGCR_SPMV_NT");

template <bool SHIFT>
static int sten_rows(const CsrDev &A, const Rows &r) {
    // window variants: 512 rows + halo <= 256 (grids up to n = 256), or 1024 rows + halo <= 512 when that catches
    // near slots the smaller one cannot (+-n of planes up to 512 wide)
    const bool tile_on = g_sten_tile.on();
    const bool big = tile_on && A.sten_near_f == 0x3eu && A.sten_halo_f > 0 && (A.sten_near != 0x3eu || A.sten_halo == 0);
    const bool small = tile_on && !big && A.sten_near == 0x3eu && A.sten_halo > 0;
    const int64_t first = r.row_begin & ~(int64_t)63, row_end = r.row_begin + r.row_count;
    const Tiles t = tiles_of(row_end - first, big ? RED_THREADS : STEN_TILE);
    RowMat m = row_mat(A, SHIFT, r.k);
    m.xh = r.xh; m.n_own = r.n_own;
    if (big || small) m.sten_halo = big ? A.sten_halo_f : A.sten_halo;
    auto go = [&](auto kernel, int blk, size_t lds) -> int {
        return launch(kernel, t.grid, blk, lds, m, r.row_begin, row_end, first, t.ntiles, t.xcd ? 1 : 0, r.x, r.y, r.w, g_skip.p, g_skip.it);
    };
    auto form = [&](auto f) -> int {   // the three forms the kernels exist in: f(slots, rare-tail layout)
        if (A.sten_rare) return f(std::integral_constant<int, 9>{}, std::true_type{});
        if (sten_slots(A) == 7) return f(std::integral_constant<int, 7>{}, std::false_type{});
        return f(std::integral_constant<int, 9>{}, std::false_type{});
    };
    return form([&](auto NS, auto RARE) -> int {
        if (!big && !small) return go(sten_spmv<decltype(NS)::value, decltype(RARE)::value, SHIFT, STEN_TILE>, STEN_TILE, 0);
        return dispatch_bool(big, [&](auto BIG) -> int {
            constexpr int BLK = decltype(BIG)::value ? RED_THREADS : STEN_TILE;
            return dispatch_bool(g_sten_dma.on() && m.sten_halo % 64 == 0, [&](auto DMA) -> int {
                return go(sten_spmv_tile<decltype(NS)::value, decltype(RARE)::value, SHIFT, BLK, 0x3eu, decltype(DMA)::value>, BLK,
                          (size_t)(BLK + 2 * m.sten_halo) * sizeof(cplx));
            });
        });
    });
}

template <bool SHIFT>
static int pat_lds_rows(const CsrDev &A, const Rows &r) {   // dictionary with values, table staged in LDS
    const Tiles t = tiles_of(r.row_count, 256);
    const size_t lds = (size_t)A.npat * A.W * (A.pat_real ? 12 : 20);
    return dispatch_value<7, 0>(A.W, [&](auto WT) -> int {
        return dispatch_bool(A.pat_real, [&](auto RV) -> int {
            return launch(pat_spmv_lds<decltype(WT)::value, SHIFT, decltype(RV)::value, 1, 256>, t.grid, 256, lds, r.row_begin, r.row_count, A.W,
                          t.ntiles, t.xcd ? 1 : 0, A.npat, A.pat_id, A.pat_off, A.pat_re, A.pat_im, r.x, r.xh, r.n_own, r.y, r.k, r.w, g_skip.p,
                          g_skip.it);
        });
    });
}

template <bool SHIFT>
static int pat_rows(const CsrDev &A, const Rows &r) {   // dictionary, table read through the caches
    const Tiles t = tiles_of(r.row_count, 256);
    const bool realv = A.pat_mode == 1 ? A.pat_real : A.ell_val_re != nullptr;
    return dispatch_value<1, 2>(A.pat_mode, [&](auto M) -> int {
        return dispatch_value<7, 0>(A.W, [&](auto WT) -> int {
            return dispatch_bool(t.xcd, [&](auto X) -> int {
                return dispatch_bool(realv, [&](auto RV) -> int {
                    return launch(pat_spmv_rowthread<decltype(WT)::value, SHIFT, decltype(X)::value, decltype(M)::value, decltype(RV)::value>, t.grid,
                                  256, 0, r.row_begin, r.row_count, A.npad, A.W, t.ntiles, A.pat_id, A.pat_off, A.pat_re, A.pat_im, slab_values(A),
                                  r.x, r.xh, r.n_own, r.y, r.k, r.w, g_skip.p, g_skip.it);
                });
            });
        });
    });
}

template <bool SHIFT>
static int window_rows(const CsrDev &A, const Rows &r) {   // whole matrix, x window in LDS
    const Tiles t = tiles_of(A.nrow, ELL_WIN_ROWS);
    const bool tail = window_fuses_tail(A);
    const size_t lds = sizeof(cplx) * (size_t)(ELL_WIN_ROWS + 2 * A.win_h + (tail ? WIN_TAIL_CH : 0));
    return dispatch_value<1024, 4096>(A.win_h, [&](auto H) -> int {
        return dispatch_bool(A.ell_val_re != nullptr, [&](auto RV) -> int {
            return dispatch_bool(tail, [&](auto TL) -> int {
                const auto kernel = ell_spmv_window<SHIFT, decltype(RV)::value, decltype(H)::value, decltype(TL)::value>;
                static bool big_lds = false;   // (one per instantiation)
                if (!big_lds) {
                    MGCR_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                    big_lds = true;
                }
                return launch(kernel, t.grid, ELL_WIN_ROWS, lds, A.nrow, A.npad, A.W, t.ntiles, slab_values(A), A.ell_col, r.x, r.y, r.k, r.w, g_skip.p,
                              g_skip.it, A.win_tile_tail, A.win_row_tail, A.tail_ptr, A.tail_col, A.tail_val);
            });
        });
    });
}

template <bool SHIFT>
static int slab_rows(const CsrDev &A, const Rows &r) {   // slab, one thread per row
    const Tiles t = tiles_of(r.row_count, 256);
    return dispatch_value<7, 0>(A.W, [&](auto WT) -> int {
        return dispatch_bool(t.xcd, [&](auto X) -> int {
            return dispatch_bool(A.ell_val_re != nullptr, [&](auto RV) -> int {
                return dispatch_bool(g_spmv_nt.on(), [&](auto NT) -> int {
                    return launch(ell_spmv_rowthread<decltype(WT)::value, SHIFT, decltype(X)::value, decltype(RV)::value, decltype(NT)::value>, t.grid,
                                  256, 0, r.row_begin, r.row_count, A.npad, A.W, t.ntiles, slab_values(A), A.ell_col, r.x, r.xh, r.n_own, r.y, r.k,
                                  r.w, g_skip.p, g_skip.it);
                });
            });
        });
    });
}

template <bool SHIFT>
static int lanes_rows(const CsrDev &A, const Rows &r) {   // slab, L = 2 .. 16 lanes per row
    const unsigned grid = (unsigned)((r.row_count * A.L + 255) / 256);
    return dispatch_value<2, 4, 8, 16>(A.L, [&](auto LL) -> int {
        return dispatch_bool(A.ell_val_re != nullptr, [&](auto RV) -> int {
            return launch(ell_spmv_lanes<decltype(LL)::value, SHIFT, decltype(RV)::value>, grid, 256, 0, r.row_begin, r.row_count, A.npad, A.nchunk,
                          slab_values(A), A.ell_col, r.x, r.xh, r.n_own, r.y, r.k, r.w, g_skip.p, g_skip.it);
        });
    });
}

template <bool SHIFT>
static int ell_rows(const CsrDev &A, int64_t row_begin, int64_t row_count, const cplx *x, const cplx *xh, int32_t n_own, cplx *y, cplx k,
                    const cplx *w) {
    if (row_count <= 0) return MGCR_OK;
    const Rows r{row_begin, row_count, x, xh, n_own, y, k, w};
    if (csr_stencil_active(A)) return sten_rows<SHIFT>(A, r);
    if (A.pat_mode == 1 && (int64_t)A.npat * A.W * 20 <= 48 * 1024) return pat_lds_rows<SHIFT>(A, r);  // pattern table fits LDS
    if (A.pat_mode) return pat_rows<SHIFT>(A, r);
    if (A.L == 1 && A.win_h && !xh && row_begin == 0 && row_count == A.nrow) return window_rows<SHIFT>(A, r);
    return A.L == 1 ? slab_rows<SHIFT>(A, r) : lanes_rows<SHIFT>(A, r);
}

// dist_halo_end for a begun exchange, also when the interior rows between the two fail to launch: the wait half of a split
// peer-write exchange is never skipped (halo.hip), or the next exchange would meet a stale pending wait
struct HaloEnd {
    DistCsr *d;
    int end() { DistCsr *q = d; d = nullptr; return dist_halo_end(q); }
    ~HaloEnd() { if (d) dist_halo_end(d); }
};

template <bool SHIFT>
static int csr_apply_t(const CsrDev &A, const cplx *x, cplx *y, cplx k, DistCsr *dist, const cplx *w) {
    if (A.nrow == 0) return MGCR_OK;
    const cplx *xh = nullptr;
    int32_t n_own = INT32_MAX;
    if (dist) {
        // halo exchange on the communication stream, overlapped with the rows that need no halo
        int64_t ib = 0, ie = 0;
        dist_info(dist, &xh, &ib, &ie);
        n_own = (int32_t)A.nrow;
        MGCR_TRY(dist_halo_begin(dist, x, ie > ib && g_spmv_part == 0));
        HaloEnd halo{dist};
        xh = dist_halo_ptr(dist);
        MGCR_TRY(ell_rows<SHIFT>(A, ib, ie - ib, x, xh, n_own, y, k, w));
        MGCR_TRY(halo.end());
        MGCR_TRY(ell_rows<SHIFT>(A, 0, ib, x, xh, n_own, y, k, w));
        MGCR_TRY(ell_rows<SHIFT>(A, ie, A.nrow - ie, x, xh, n_own, y, k, w));
    } else if (g_spmv_part != 2) {
        // 256 x 256 x Z grids: the carried-window form (gcr_fused.hip) — every entry of x requested once, no far gathers
        if (g_spmv_part == 0 && csr_stencil_active(A) && csr_apply_carry(A, x, y, SHIFT, k, w)) return MGCR_OK;
        MGCR_TRY(ell_rows<SHIFT>(A, 0, A.nrow, x, xh, n_own, y, k, w));
    }
    if (A.n_tail_rows && g_spmv_part != 1) {
        if (A.n_tail_chunks && !(window_fuses_tail(A) && !dist)) {
            MGCR_TRY(launch(csr_tail_chunk_kernel<SHIFT>, (unsigned)A.n_tail_chunks, TAIL_THREADS, 0, A.tail_chunk, A.tail_rows, A.tail_ptr, A.tail_col,
                            A.tail_val, x, xh, n_own, y, k, g_skip.p, g_skip.it));
        }
        if (A.n_tail_long) {
            int64_t threads = (int64_t)A.n_tail_long * 64;
            MGCR_TRY(launch(csr_tail_kernel<SHIFT>, (unsigned)((threads + 255) / 256), 256, 0, (int64_t)A.n_tail_long, A.tail_long, A.tail_rows,
                            A.tail_ptr, A.tail_col, A.tail_val, x, xh, n_own, y, k, w, g_skip.p, g_skip.it));
        }
    }
    return MGCR_OK;
}

int csr_apply(const CsrDev &A, const cplx *x, cplx *y, bool shift, cplx k, DistCsr *dist, const cplx *w) {
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "SpMV cannot run in place");
    MGCR_CHECK(!w || (shift && w != y), MGCR_ERR_INVALID, "csr_apply: w needs the shifted form and its own storage");
    return shift ? csr_apply_t<true>(A, x, y, k, dist, w) : csr_apply_t<false>(A, x, y, k, dist, nullptr);
}

// ------------------------------------------------------------------------------------------------
// block-CSR of dense bs x bs blocks (HierarchicalSparse).  One wave per block-row.  Per block the
// wave streams the bs*bs entries with coalesced 16-B loads, stages the products m[r][c]*x[c] in
// LDS, and lanes r < bs then add their row's products in column order — the order of
// Dense::operator() (src/Operator.h:165-170) — onto the block-row accumulator
// (value += ..., src/HierarchicalSparse.h:144).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) bcsr_wave_kernel(int32_t nbrow, int32_t bs, const int32_t *__restrict__ browptr,
                                                       const int32_t *__restrict__ bcol, const cplx *__restrict__ blocks,
                                                       const cplx *__restrict__ x, const cplx *__restrict__ xh, int32_t nb_own,
                                                       cplx *__restrict__ y, const int *__restrict__ skip, int skip_it, const int32_t *__restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cplx *prod = reinterpret_cast<cplx *>(smem_raw);  // [bs][bs+1]
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    const int32_t brow = order ? order[blockIdx.x] : (int32_t)blockIdx.x;   // longest block rows first (bcsr_build_device)
    const int lane = threadIdx.x;
    const int32_t bs2 = bs * bs, ld = bs + 1;
    const int32_t beg = browptr[brow], end = browptr[brow + 1];
    // rows of a block owned by this lane: r = lane, lane+64 (bs <= 128)
    cplx acc0 = make_double2(0., 0.), acc1 = make_double2(0., 0.);
    for (int32_t l = beg; l < end; l++) {
        const cplx *m = blocks + (int64_t)l * bs2;
        const int32_t bc = bcol[l];
        const cplx *xb = bc < nb_own ? x + (int64_t)bc * bs : xh + (int64_t)(bc - nb_own) * bs;
        for (int32_t e = lane; e < bs2; e += 64) {
            int32_t r = e / bs, cc = e - r * bs;
            prod[r * ld + cc] = cmul(m[e], xb[cc]);
        }
        __syncthreads();
        if (lane < bs) {
            cplx o = make_double2(0., 0.);
            for (int32_t cc = 0; cc < bs; cc++) o = cadd(o, prod[lane * ld + cc]);
            acc0 = cadd(acc0, o);
        }
        if (lane + 64 < bs) {
            cplx o = make_double2(0., 0.);
            for (int32_t cc = 0; cc < bs; cc++) o = cadd(o, prod[(lane + 64) * ld + cc]);
            acc1 = cadd(acc1, o);
        }
        __syncthreads();
    }
    if (lane < bs) y[(int64_t)brow * bs + lane] = acc0;
    if (lane + 64 < bs) y[(int64_t)brow * bs + lane + 64] = acc1;
}

// Same algorithm with the block's bs*bs entries held in registers: TT = ceil(bs*bs/64) (rounded up to
// 1, 2, 4, 8, 16) matrix loads and x gathers per lane are ISSUED TOGETHER for every block, instead of
// one dependent load per loop trip — the generic kernel above keeps a single 1-KiB load in flight per
// wave and is latency-bound.  The (row, column) of each lane's entries does not depend on the block
// and is computed once.  PREFETCH additionally keeps the NEXT block's loads in flight during the LDS
// phase; measured on MI355X (bs = 20, 3 GB of blocks) it loses to the plain form (5.08 vs 5.28 TB/s:
// 164 VGPRs cost a third of the resident waves), so it is compiled but not dispatched.
template <int TT, bool PREFETCH>
__global__ void __launch_bounds__(64) bcsr_wave_kernel_t(int32_t nbrow, int32_t bs, const int32_t *__restrict__ browptr,
                                                         const int32_t *__restrict__ bcol, const cplx *__restrict__ blocks,
                                                         const cplx *__restrict__ x, const cplx *__restrict__ xh, int32_t nb_own,
                                                         cplx *__restrict__ y, const int *__restrict__ skip, int skip_it, const int32_t *__restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cplx *prod = reinterpret_cast<cplx *>(smem_raw);  // [bs][bs+1]
    if (skip && skip[0] < skip[1] + skip_it) return;  // {stop_at, base}: see gcr.hip DevState
    const int32_t brow = order ? order[blockIdx.x] : (int32_t)blockIdx.x;   // longest block rows first (bcsr_build_device)
    const int lane = threadIdx.x;
    const int32_t bs2 = bs * bs, ld = bs + 1;
    const int32_t beg = browptr[brow], end = browptr[brow + 1];
    int32_t ecol[TT], elds[TT];
    bool live[TT];
#pragma unroll
    for (int t = 0; t < TT; t++) {
        int32_t e = lane + 64 * t;
        live[t] = e < bs2;
        int32_t r = live[t] ? e / bs : 0;
        ecol[t] = live[t] ? e - r * bs : 0;
        elds[t] = r * ld + ecol[t];
    }
    cplx acc = make_double2(0., 0.);
    cplx mv[TT], xv[TT], mn[TT], xn[TT];
    auto fetch = [&](int32_t l, cplx (&mo)[TT], cplx (&xo)[TT]) {
        const cplx *m = blocks + (int64_t)l * bs2;
        const int32_t bc = bcol[l];
        const cplx *xb = bc < nb_own ? x + (int64_t)bc * bs : xh + (int64_t)(bc - nb_own) * bs;
#pragma unroll
        for (int t = 0; t < TT; t++) {
            mo[t] = live[t] ? m[lane + 64 * t] : make_double2(0., 0.);
            xo[t] = xb[ecol[t]];
        }
    };
    if (beg < end) fetch(beg, mv, xv);
    for (int32_t l = beg; l < end; l++) {
        // the next block's loads are in flight while this block goes through LDS
        if (PREFETCH && l + 1 < end) fetch(l + 1, mn, xn);
#pragma unroll
        for (int t = 0; t < TT; t++)
            if (live[t]) prod[elds[t]] = cmul(mv[t], xv[t]);
        __syncthreads();
        if (lane < bs) {
            cplx o = make_double2(0., 0.);
            for (int32_t cc = 0; cc < bs; cc++) o = cadd(o, prod[lane * ld + cc]);
            acc = cadd(acc, o);
        }
        __syncthreads();
        if (PREFETCH) {
#pragma unroll
            for (int t = 0; t < TT; t++) { mv[t] = mn[t]; xv[t] = xn[t]; }
        } else if (l + 1 < end) {
            fetch(l + 1, mv, xv);
        }
    }
    if (lane < bs) y[(int64_t)brow * bs + lane] = acc;
}

int bcsr_apply(const BcsrDev &A, const cplx *x, cplx *y, const cplx *xh, int32_t nb_own) {
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "block SpMV cannot run in place");
    if (A.nbrow == 0) return MGCR_OK;
    size_t lds = sizeof(cplx) * (size_t)A.bs * (size_t)(A.bs + 1);
    static bool attr_set = false;
    if (!attr_set) {
        MGCR_HIP(hipFuncSetAttribute((const void *)bcsr_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    MGCR_CHECK(lds <= 160 * 1024, MGCR_ERR_UNSUPPORTED, "block size %d needs more than 160 KiB of LDS", A.bs);
    auto go = [&](auto kernel) -> int {
        return launch(kernel, (unsigned)A.nbrow, 64, lds, A.nbrow, A.bs, A.browptr, A.bcol, A.blocks, x, xh, nb_own, y, g_skip.p, g_skip.it, A.order);
    };
    const int tt = (A.bs * A.bs + 63) / 64;   // matrix loads per lane, rounded up to 1, 2, 4, 8, 16
    if (A.bs > 64 || tt > 16) return go(bcsr_wave_kernel);  // rows beyond lane 63 / too many registers: generic kernel
    return dispatch_value<1, 2, 4, 8, 16>(tt <= 2 ? tt : tt <= 4 ? 4 : tt <= 8 ? 8 : 16,
                                          [&](auto TT) -> int { return go(bcsr_wave_kernel_t<decltype(TT)::value, false>); });
}

// For spmv_build.hip ell_window_try; kept in this file: compiled in that one its shuffle tree comes out with other instructions.
// How local are the slab's columns?  (count of slots within 1024 / 4096 rows of their row)
__global__ void __launch_bounds__(256) ell_band_count_kernel(int64_t nrow, int64_t npad, int32_t W, const int32_t *__restrict__ col,
                                                             unsigned long long *__restrict__ cnt) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long c1 = 0, c4 = 0;
    if (row < nrow)
        for (int32_t w = 0; w < W; w++) {
            const int64_t d = (int64_t)col[(int64_t)w * npad + row] - row;
            const int64_t a = d < 0 ? -d : d;
            c1 += a <= 1024;
            c4 += a <= 4096;
        }
    // wave totals, then one atomic per wave and counter
    for (int off = 32; off >= 1; off >>= 1) {
        c1 += __shfl_down(c1, off, 64);
        c4 += __shfl_down(c4, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(cnt, c1);
        atomicAdd(cnt + 1, c4);
    }
}
int ell_band_count(const CsrDev &A, unsigned long long *d_cnt) {
    return launch(ell_band_count_kernel, (unsigned)((A.nrow + 255) / 256), 256, 0, A.nrow, A.npad, A.W, A.ell_col, d_cnt);
}

}  // namespace mgcr
