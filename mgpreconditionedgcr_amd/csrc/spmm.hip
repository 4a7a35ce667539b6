// k-wide operator apply: Y = A X for a block of k Fields stored with the columns interleaved (multi_dev.h), so that the
// matrix is streamed ONCE for all k products and one gathered row of X is k contiguous values (k = 8: one 128-byte line).
//
// Rule for the arithmetic: column j of Y is bit-identical to the single apply (spmv.hip) on column j.  Every kernel below
// keeps, per column, the order in which the single kernels add a row's products — ELL slab: lane l of L adds entries
// l, l + L, ... and the L sums go through the shfl_down tree; tail: CSR order onto a tail sum that is then added to the row
// (chunk rows), 64 lanes striding + wave tree (rows longer than a chunk); block-CSR: a block's products of a row in column
// order, blocks in storage order; dictionary / stencil view: row_product / sten_row_product of spmv_dev.h called per column.
// No fused multiply-adds (-ffp-contract=off), no MFMA.
//
// The shift y = w - k (A x) comes in two forms (multi_dev.h): KUniform, one k for every column (Sparse residual form, DiracOp), and
// KCols, one k PER COLUMN (MultiDiracOp: 16 values in the kernel arguments, so a launch carries the values of the moment it was
// enqueued).  Every Sparse kernel below is a body templated on that type and two __global__ entries: NAME<...> with the uniform k —
// the kernels as they were, name and arguments — and NAME_kcol<...> with the per-column values (256 bytes more of kernel
// arguments, which the small operators' launch-bound applies would pay for: measured).  The expression per
// column is the single kernels' csub(w, cmul(k_j, sum)) either way.
#include "internal.h"
#include "reduce.h"
#include "spmv_dev.h"
#include "multi_dev.h"

namespace mgcr {

// ------------------------------------------------------------------------------------------------
// ELL slab.  A thread (L = 1) or a group of L = 1 << lshift lanes owns a row for ALL k columns: every (col, val) is read once
// (non-temporally: the slab is touched once per apply), the k values of X's row `col` are one contiguous 16 k-byte piece, and
// the thread keeps K >= k accumulators.  MASK: k < K, the columns beyond k are neither loaded nor stored.
// ------------------------------------------------------------------------------------------------
template <int K, bool MASK, bool REALV, typename KS>
__device__ __forceinline__ void ell_multi_body(int64_t nrow, int64_t npad, int32_t nchunk, int lshift, const void *__restrict__ val,
                                               const int32_t *__restrict__ col, const cplx *__restrict__ x, cplx *__restrict__ y,
                                               int k, int shift, const KS ks, const cplx *__restrict__ w) {
    const int L = 1 << lshift;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t >> lshift;
    const int l = (int)(t & (L - 1));
    cplx sum[K];
#pragma unroll
    for (int q = 0; q < K; q++) sum[q] = make_double2(0., 0.);
    if (row < nrow) {
#pragma unroll 2
        for (int32_t c = 0; c < nchunk; c++) {
            const int64_t idx = (((int64_t)c * npad + row) << lshift) + l;
            const int32_t j = ldcol<true>(col + idx);
            const cplx *xr = x + (int64_t)j * k;
            cplx xv[K];
#pragma unroll
            for (int q = 0; q < K; q++) xv[q] = (!MASK || q < k) ? xr[q] : make_double2(0., 0.);
            if (REALV) {
                const double v = __builtin_nontemporal_load(reinterpret_cast<const double *>(val) + idx);
#pragma unroll
                for (int q = 0; q < K; q++) sum[q] = cadd(sum[q], make_double2(v * xv[q].x, v * xv[q].y));
            } else {
                const cplx *p = reinterpret_cast<const cplx *>(val) + idx;
                const cplx v = make_double2(__builtin_nontemporal_load(&p->x), __builtin_nontemporal_load(&p->y));
#pragma unroll
                for (int q = 0; q < K; q++) sum[q] = cadd(sum[q], cmul(v, xv[q]));
            }
        }
    }
    for (int off = L >> 1; off >= 1; off >>= 1) {   // (no trip for L = 1)
#pragma unroll
        for (int q = 0; q < K; q++) {
            sum[q].x += __shfl_down(sum[q].x, off, L);
            sum[q].y += __shfl_down(sum[q].y, off, L);
        }
    }
    if (row < nrow && l == 0) {
        const cplx *wr = (w ? w : x) + row * k;
#pragma unroll
        for (int q = 0; q < K; q++)
            if (!MASK || q < k) y[row * k + q] = shift ? csub(wr[q], cmul(ks.at(q), sum[q])) : sum[q];
    }
}
template <int K, bool MASK, bool REALV>
__global__ void __launch_bounds__(256) ell_multi_kernel(int64_t nrow, int64_t npad, int32_t nchunk, int lshift, const void *__restrict__ val,
                                                        const int32_t *__restrict__ col, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                        int k, int shift, cplx kk, const cplx *__restrict__ w) {
    ell_multi_body<K, MASK, REALV>(nrow, npad, nchunk, lshift, val, col, x, y, k, shift, KUniform{kk}, w);
}
template <int K, bool MASK, bool REALV>
__global__ void __launch_bounds__(256) ell_multi_kernel_kcol(int64_t nrow, int64_t npad, int32_t nchunk, int lshift, const void *__restrict__ val,
                                                             const int32_t *__restrict__ col, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                             int k, int shift, KCols ks, const cplx *__restrict__ w) {
    ell_multi_body<K, MASK, REALV>(nrow, npad, nchunk, lshift, val, col, x, y, k, shift, ks, w);
}

// CSR tail, the rows of a chunk: the k-wide form of csr_tail_chunk_kernel.  One workgroup per chunk (a run of consecutive tail
// rows with at most TAIL_CAP entries and TAIL_THREADS rows).  The chunk's entries are one contiguous piece of the tail arrays:
// the workgroup streams it TAIL_THREADS entries per trip with coalesced, non-temporal loads (the next trip's columns and values
// are requested before this trip's products are formed), every thread gathers the k contiguous values of X's row `col` and
// stages its k products in LDS, prod[K][TAIL_THREADS]; thread t then adds the trip's products of ITS row, per column, in CSR
// order onto the row's tail sum, which is added to the row's ELL sum at the end — csr_tail_chunk_kernel's order, same bits.
template <int K, typename KS>
__device__ __forceinline__ void tail_chunk_multi_body(const int4 *__restrict__ chunks, const int32_t *__restrict__ tail_rows,
                                                      const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                      const cplx *__restrict__ tail_val, const cplx *__restrict__ x,
                                                      cplx *__restrict__ y, int k, int shift, const KS ks, int c0, int kw) {
    // (columns [c0, c0 + kw) of the k, kw <= K; ks.at(q) is the shift of column c0 + q — the host passes the window's values, so
    // that every index into the kernel arguments is a constant: 12 columns run as 8 + 4 — the 16-wide form's 64 KB of products and 210 registers
    // leave 2 waves per SIMD and measured slower than streaming the tail twice)
    __shared__ cplx prod[K * TAIL_THREADS];
    const int t = threadIdx.x;
    const int4 ch = chunks[blockIdx.x];
    const int32_t r0 = ch.x, r1 = ch.y, e0 = ch.z, e1 = ch.w;
    const bool has_row = r0 + t < r1;
    int32_t rb = 0, re = 0;
    int64_t row = 0;
    if (has_row) { rb = tail_ptr[r0 + t]; re = tail_ptr[r0 + t + 1]; row = tail_rows[r0 + t]; }
    cplx sum[K];
#pragma unroll
    for (int q = 0; q < K; q++) sum[q] = make_double2(0., 0.);
    int32_t jn = -1;
    cplx vn = make_double2(0., 0.);
    auto fetch = [&](int32_t cb) {
        const int32_t e = cb + t;
        jn = -1;
        vn = make_double2(0., 0.);
        if (e < e1) {
            jn = __builtin_nontemporal_load(tail_col + e);
            vn = make_double2(__builtin_nontemporal_load(&tail_val[e].x), __builtin_nontemporal_load(&tail_val[e].y));
        }
    };
    if (e0 < e1) fetch(e0);
    for (int32_t cb = e0; cb < e1; cb += TAIL_THREADS) {   // uniform trip count
        const int32_t jc = jn;
        const cplx vc = vn;
        cplx xv[K];
        if (jc >= 0) {
            const cplx *xr = x + (int64_t)jc * k + c0;
#pragma unroll
            for (int q = 0; q < K; q++) xv[q] = q < kw ? xr[q] : make_double2(0., 0.);
        }
        if (cb + TAIL_THREADS < e1) fetch(cb + TAIL_THREADS);
        if (jc >= 0) {
#pragma unroll
            for (int q = 0; q < K; q++) prod[q * TAIL_THREADS + t] = cmul(vc, xv[q]);
        }
        __syncthreads();
        const int32_t ib = (rb > cb ? rb : cb) - cb, ie = (re < cb + TAIL_THREADS ? re : cb + TAIL_THREADS) - cb;
        for (int32_t i = ib; i < ie; i++) {
#pragma unroll
            for (int q = 0; q < K; q++) sum[q] = cadd(sum[q], prod[q * TAIL_THREADS + i]);
        }
        __syncthreads();
    }
    if (has_row) {
#pragma unroll
        for (int q = 0; q < K; q++)
            if (q < kw) {
                const cplx y0 = y[row * k + c0 + q];
                y[row * k + c0 + q] = shift ? csub(y0, cmul(ks.at(q), sum[q])) : cadd(y0, sum[q]);
            }
    }
}
template <int K>
__global__ void __launch_bounds__(TAIL_THREADS) tail_chunk_multi_kernel(const int4 *__restrict__ chunks, const int32_t *__restrict__ tail_rows,
                                                                        const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                                        const cplx *__restrict__ tail_val, const cplx *__restrict__ x,
                                                                        cplx *__restrict__ y, int k, int shift, cplx kk, int c0, int kw) {
    tail_chunk_multi_body<K>(chunks, tail_rows, tail_ptr, tail_col, tail_val, x, y, k, shift, KUniform{kk}, c0, kw);
}
template <int K>
__global__ void __launch_bounds__(TAIL_THREADS) tail_chunk_multi_kernel_kcol(const int4 *__restrict__ chunks, const int32_t *__restrict__ tail_rows,
                                                                             const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                                             const cplx *__restrict__ tail_val, const cplx *__restrict__ x,
                                                                             cplx *__restrict__ y, int k, int shift, KCols ks, int c0, int kw) {
    tail_chunk_multi_body<K>(chunks, tail_rows, tail_ptr, tail_col, tail_val, x, y, k, shift, ks, c0, kw);
}

// CSR tail, rows longer than a chunk (csr_tail_kernel's): one wave per row, lanes stride the entries, wave tree per column
template <int K, typename KS>
__device__ __forceinline__ void tail_long_multi_body(int64_t n_long, const int32_t *__restrict__ tail_long, const int32_t *__restrict__ tail_rows,
                                                     const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                     const cplx *__restrict__ tail_val, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                     int k, int shift, const KS ks) {
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= n_long) return;
    const int32_t t = tail_long[wave];
    const int32_t beg = tail_ptr[t], end = tail_ptr[t + 1];
    cplx sum[K];
#pragma unroll
    for (int q = 0; q < K; q++) sum[q] = make_double2(0., 0.);
    for (int32_t i = beg + lane; i < end; i += 64) {
        const cplx v = tail_val[i];
        const cplx *xr = x + (int64_t)tail_col[i] * k;
#pragma unroll
        for (int q = 0; q < K; q++)
            if (q < k) sum[q] = cadd(sum[q], cmul(v, xr[q]));
    }
#pragma unroll
    for (int q = 0; q < K; q++) {
        sum[q].x = wave_sum(sum[q].x);
        sum[q].y = wave_sum(sum[q].y);
    }
    if (lane == 0) {
        const int64_t row = tail_rows[t];
#pragma unroll
        for (int q = 0; q < K; q++)
            if (q < k) {
                const cplx y0 = y[row * k + q];
                y[row * k + q] = shift ? csub(y0, cmul(ks.at(q), sum[q])) : cadd(y0, sum[q]);
            }
    }
}
template <int K>
__global__ void __launch_bounds__(256) tail_long_multi_kernel(int64_t n_long, const int32_t *__restrict__ tail_long, const int32_t *__restrict__ tail_rows,
                                                              const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                              const cplx *__restrict__ tail_val, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                              int k, int shift, cplx kk) {
    tail_long_multi_body<K>(n_long, tail_long, tail_rows, tail_ptr, tail_col, tail_val, x, y, k, shift, KUniform{kk});
}
template <int K>
__global__ void __launch_bounds__(256) tail_long_multi_kernel_kcol(int64_t n_long, const int32_t *__restrict__ tail_long, const int32_t *__restrict__ tail_rows,
                                                                   const int32_t *__restrict__ tail_ptr, const int32_t *__restrict__ tail_col,
                                                                   const cplx *__restrict__ tail_val, const cplx *__restrict__ x, cplx *__restrict__ y,
                                                                   int k, int shift, KCols ks) {
    tail_long_multi_body<K>(n_long, tail_long, tail_rows, tail_ptr, tail_col, tail_val, x, y, k, shift, ks);
}

// Row-pattern dictionary (MODE 1: offsets and values in the table, 2: offsets only) and stencil view (MODE 3; RARE: the
// rare-tail layout): ONE generic row-thread kernel, the single kernels' row product (spmv_dev.h) called once per column
// through its x hook.  Correct and bit-exact; not tuned (the table / presence words are re-read per column, from cache).
template <int MODE, int NS, bool RARE, typename KS>
__device__ __forceinline__ void rowgen_multi_body(const RowMat &m, int64_t nrow, const cplx *__restrict__ x, cplx *__restrict__ y, int k,
                                                  const KS ks, const cplx *__restrict__ w) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((row & ~(int64_t)63) >= nrow) return;   // the whole wave lies outside
    const bool live = row < nrow;
    const int64_t r = live ? row : nrow - 1;
    const PatLds pl{m.poff, m.pre, m.pim};      // (the table is read where it lies)
    int32_t t0 = 0;
    if (MODE == 1 || MODE == 2) t0 = (int32_t)m.pid[r] * m.W;
    for (int q = 0; q < k; q++) {
        auto xf = [&](int32_t j) -> cplx { return x[(int64_t)j * k + q]; };
        cplx sum;
        if constexpr (MODE == 3) sum = sten_row_product<NS, RARE>(m, row, xf);   // (a wave holds 64 consecutive rows from a multiple of 64)
        else sum = row_product<MODE, 0>(m, r, t0, pl, xf);
        if (live) y[row * k + q] = m.shift ? csub((w ? w : x)[row * k + q], cmul(ks.at(q), sum)) : sum;
    }
}
template <int MODE, int NS, bool RARE>
__global__ void __launch_bounds__(256) rowgen_multi_kernel(RowMat m, int64_t nrow, const cplx *__restrict__ x, cplx *__restrict__ y, int k,
                                                           const cplx *__restrict__ w) {
    rowgen_multi_body<MODE, NS, RARE>(m, nrow, x, y, k, KUniform{m.k}, w);
}
template <int MODE, int NS, bool RARE>
__global__ void __launch_bounds__(256) rowgen_multi_kernel_kcol(RowMat m, int64_t nrow, const cplx *__restrict__ x, cplx *__restrict__ y, int k,
                                                                KCols ks, const cplx *__restrict__ w) {
    rowgen_multi_body<MODE, NS, RARE>(m, nrow, x, y, k, ks, w);
}

template <bool REALV>
static int launch_ell_multi(const CsrDev &A, const cplx *x, cplx *y, int k, int shift, cplx kk, const KCols *kc, const cplx *w) {
    int lshift = 0;
    while ((1 << lshift) < A.L) lshift++;
    const int64_t threads = A.nrow << lshift;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    const void *vals = A.ell_val_re ? (const void *)A.ell_val_re : (const void *)A.ell_val;
#define EM(KK, MM)                                                                                                                  \
    do {                                                                                                                            \
        if (kc)                                                                                                                     \
            hipLaunchKernelGGL((ell_multi_kernel_kcol<KK, MM, REALV>), dim3(grid), dim3(256), 0, ctx().stream, A.nrow, A.npad, A.nchunk, lshift, \
                               vals, (const int32_t *)A.ell_col, x, y, k, shift, *kc, w);                                           \
        else                                                                                                                        \
            hipLaunchKernelGGL((ell_multi_kernel<KK, MM, REALV>), dim3(grid), dim3(256), 0, ctx().stream, A.nrow, A.npad, A.nchunk, lshift, \
                               vals, (const int32_t *)A.ell_col, x, y, k, shift, kk, w);                                            \
    } while (0)
    switch (k) {
        case 1: EM(1, false); break;
        case 2: EM(2, false); break;
        case 3: EM(4, true); break;
        case 4: EM(4, false); break;
        case 8: EM(8, false); break;
        case 12: EM(12, false); break;
        case 16: EM(16, false); break;
        default:
            if (k < 8) EM(8, true);
            else if (k < 12) EM(12, true);
            else EM(16, true);
            break;
    }
#undef EM
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

// entry q = the shift of column c0 + q (entries past column 15 repeat the last one; no kernel reads them)
static KCols kcols_window(const KCols &ks, int c0) {
    KCols w;
    for (int q = 0; q < MV_MAX_K; q++) w.v[q] = ks.v[c0 + q < MV_MAX_K ? c0 + q : MV_MAX_K - 1];
    return w;
}

// kc == nullptr: the uniform shift kk; else the shift per column (kk unused)
int csr_apply_multi(const CsrDev &A, const cplx *x, cplx *y, int k, bool shift, cplx kk, const KCols *kc, const cplx *w) {
    Context &c = ctx();
    if (A.nrow == 0) return MGCR_OK;
    const unsigned rgrid = (unsigned)((A.nrow + 255) / 256);
    if (csr_stencil_active(A) || A.pat_mode) {
        const RowMat m = row_mat(A, shift, kk);   // (the per-column kernel takes its shifts from *kc, not from m.k)
#define RG(MODE, NS, RARE)                                                                                                                   \
    do {                                                                                                                                     \
        if (kc) hipLaunchKernelGGL((rowgen_multi_kernel_kcol<MODE, NS, RARE>), dim3(rgrid), dim3(256), 0, c.stream, m, A.nrow, x, y, k, *kc, w); \
        else hipLaunchKernelGGL((rowgen_multi_kernel<MODE, NS, RARE>), dim3(rgrid), dim3(256), 0, c.stream, m, A.nrow, x, y, k, w);           \
    } while (0)
        if (csr_stencil_active(A)) {
            if (A.sten_rare) RG(3, 9, true);
            else if (sten_slots(A) == 7) RG(3, 7, false);
            else RG(3, 9, false);
        } else if (A.pat_mode == 1) RG(1, 0, false);
        else RG(2, 0, false);
#undef RG
        MGCR_HIP(hipGetLastError());
    } else if (A.ell_val_re) {
        MGCR_TRY(launch_ell_multi<true>(A, x, y, k, shift ? 1 : 0, kk, kc, w));
    } else {
        MGCR_TRY(launch_ell_multi<false>(A, x, y, k, shift ? 1 : 0, kk, kc, w));
    }
    if (A.n_tail_rows) {
#define TCH(KK, C0, KW)                                                                                                                 \
    do {                                                                                                                                \
        if (kc)                                                                                                                         \
            hipLaunchKernelGGL((tail_chunk_multi_kernel_kcol<KK>), dim3((unsigned)A.n_tail_chunks), dim3(TAIL_THREADS), 0, c.stream,    \
                               (const int4 *)A.tail_chunk, (const int32_t *)A.tail_rows, (const int32_t *)A.tail_ptr,                   \
                               (const int32_t *)A.tail_col, (const cplx *)A.tail_val, x, y, k, shift ? 1 : 0, kcols_window(*kc, C0), C0, KW); \
        else                                                                                                                            \
            hipLaunchKernelGGL((tail_chunk_multi_kernel<KK>), dim3((unsigned)A.n_tail_chunks), dim3(TAIL_THREADS), 0, c.stream,         \
                               (const int4 *)A.tail_chunk, (const int32_t *)A.tail_rows, (const int32_t *)A.tail_ptr,                   \
                               (const int32_t *)A.tail_col, (const cplx *)A.tail_val, x, y, k, shift ? 1 : 0, kk, C0, KW);              \
    } while (0)
        if (A.n_tail_chunks) {
            if (k <= 2) TCH(2, 0, k);
            else if (k <= 4) TCH(4, 0, k);
            else if (k <= 8) TCH(8, 0, k);
            else {                                  // 9 .. 16 columns: 8 + the rest
                TCH(8, 0, 8);
                if (k - 8 <= 2) TCH(2, 8, k - 8);
                else if (k - 8 <= 4) TCH(4, 8, k - 8);
                else TCH(8, 8, k - 8);
            }
        }
#undef TCH
#define TK(KK)                                                                                                                              \
    do {                                                                                                                                    \
        if (A.n_tail_long && kc)                                                                                                            \
            hipLaunchKernelGGL((tail_long_multi_kernel_kcol<KK>), dim3((unsigned)(((int64_t)A.n_tail_long * 64 + 255) / 256)), dim3(256), 0, \
                               c.stream, (int64_t)A.n_tail_long, (const int32_t *)A.tail_long, (const int32_t *)A.tail_rows,                \
                               (const int32_t *)A.tail_ptr, (const int32_t *)A.tail_col, (const cplx *)A.tail_val, x, y, k, shift ? 1 : 0, *kc); \
        else if (A.n_tail_long)                                                                                                             \
            hipLaunchKernelGGL((tail_long_multi_kernel<KK>), dim3((unsigned)(((int64_t)A.n_tail_long * 64 + 255) / 256)), dim3(256), 0,     \
                               c.stream, (int64_t)A.n_tail_long, (const int32_t *)A.tail_long, (const int32_t *)A.tail_rows,                \
                               (const int32_t *)A.tail_ptr, (const int32_t *)A.tail_col, (const cplx *)A.tail_val, x, y, k, shift ? 1 : 0, kk); \
    } while (0)
        if (k <= 2) TK(2);
        else if (k <= 4) TK(4);
        else if (k <= 8) TK(8);
        else TK(16);
#undef TK
        MGCR_HIP(hipGetLastError());
    }
    return MGCR_OK;
}

// ------------------------------------------------------------------------------------------------
// Block-CSR.  One wave per block row as in bcsr_wave_kernel_t; a block's bs * bs entries are loaded ONCE into registers
// (TT per lane; TT = 0: blocks of more than 1024 entries are re-read per column group, from cache) and multiplied with the k
// columns of X's block row in groups of kg columns: the group's products go through LDS, prod[kg][bs][bs + 1], and lane
// (column jj, row r) adds its row's products in column order onto the accumulator of (row r, column jj), which lives in LDS
// as well (acc[bs][k]: no per-lane register array whose size depends on k).  kg = min(k, 64 / bs) >= 1 — one (column, row)
// pair per lane and pass.
// ------------------------------------------------------------------------------------------------
template <int TT>
__global__ void __launch_bounds__(64) bcsr_multi_kernel(int32_t nbrow, int32_t bs, const int32_t *__restrict__ browptr,
                                                        const int32_t *__restrict__ bcol, const cplx *__restrict__ blocks,
                                                        const cplx *__restrict__ x, cplx *__restrict__ y, int k, int kg,
                                                        const int32_t *__restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int32_t bs2 = bs * bs, ld = bs + 1, pstride = bs * ld;
    cplx *prod = reinterpret_cast<cplx *>(smem_raw);   // [kg][bs][bs + 1]
    cplx *acc = prod + (size_t)kg * pstride;           // [bs][k]
    const int32_t brow = order ? order[blockIdx.x] : (int32_t)blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t beg = browptr[brow], end = browptr[brow + 1];
    constexpr int TR = TT ? TT : 1;
    int32_t ecol[TR], elds[TR];
    bool live[TR];
    cplx mv[TR];
#pragma unroll
    for (int t = 0; t < TR; t++) {
        const int32_t e = lane + 64 * t;
        live[t] = TT && e < bs2;
        const int32_t r = live[t] ? e / bs : 0;
        ecol[t] = live[t] ? e - r * bs : 0;
        elds[t] = r * ld + ecol[t];
    }
    for (int32_t idx = lane; idx < bs * k; idx += 64) acc[idx] = make_double2(0., 0.);
    auto fetch = [&](int32_t l) {
        const cplx *m = blocks + (int64_t)l * bs2;
#pragma unroll
        for (int t = 0; t < TR; t++)
            mv[t] = live[t] ? make_double2(__builtin_nontemporal_load(&m[lane + 64 * t].x), __builtin_nontemporal_load(&m[lane + 64 * t].y))
                            : make_double2(0., 0.);
    };
    if (TT && beg < end) fetch(beg);
    __syncthreads();
    for (int32_t l = beg; l < end; l++) {
        const cplx *m = blocks + (int64_t)l * bs2;
        const cplx *xb = x + (int64_t)bcol[l] * bs * k;
        for (int p0 = 0; p0 < k; p0 += kg) {
            const int ng = k - p0 < kg ? k - p0 : kg;
            if (TT) {
                for (int jj = 0; jj < ng; jj++) {
#pragma unroll
                    for (int t = 0; t < TR; t++)
                        if (live[t]) prod[jj * pstride + elds[t]] = cmul(mv[t], xb[ecol[t] * k + p0 + jj]);
                }
            } else {
                for (int32_t e = lane; e < bs2; e += 64) {
                    const int32_t r = e / bs, cc = e - r * bs;
                    const cplx me = m[e];
                    for (int jj = 0; jj < ng; jj++) prod[jj * pstride + r * ld + cc] = cmul(me, xb[cc * k + p0 + jj]);
                }
            }
            __syncthreads();
            for (int32_t pi = lane; pi < ng * bs; pi += 64) {
                const int32_t jj = pi / bs, r = pi - jj * bs;
                const cplx *pr = prod + jj * pstride + r * ld;
                cplx o = make_double2(0., 0.);
                for (int32_t cc = 0; cc < bs; cc++) o = cadd(o, pr[cc]);
                acc[r * k + p0 + jj] = cadd(acc[r * k + p0 + jj], o);
            }
            __syncthreads();
        }
        if (TT && l + 1 < end) fetch(l + 1);
    }
    cplx *yb = y + (int64_t)brow * bs * k;
    for (int32_t idx = lane; idx < bs * k; idx += 64) yb[idx] = acc[idx];   // one contiguous piece of Y
}

static int bcsr_apply_multi(const BcsrDev &A, const cplx *x, cplx *y, int k) {
    if (A.nbrow == 0) return MGCR_OK;
    int kg = 64 / A.bs;
    if (kg < 1) kg = 1;
    if (kg > k) kg = k;
    const size_t lds = sizeof(cplx) * ((size_t)kg * A.bs * (A.bs + 1) + (size_t)A.bs * k);
    MGCR_CHECK(lds <= 160 * 1024, MGCR_ERR_UNSUPPORTED, "block size %d with %d columns needs more than 160 KiB of LDS", A.bs, k);
    const int tt = (A.bs * A.bs + 63) / 64;
#define BM(T_)                                                                                                                          \
    do {                                                                                                                                \
        static bool attr_set = false;                                                                                                   \
        if (!attr_set) {                                                                                                                \
            MGCR_HIP(hipFuncSetAttribute((const void *)bcsr_multi_kernel<T_>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
            attr_set = true;                                                                                                            \
        }                                                                                                                               \
        hipLaunchKernelGGL((bcsr_multi_kernel<T_>), dim3((unsigned)A.nbrow), dim3(64), lds, ctx().stream, A.nbrow, A.bs,               \
                           (const int32_t *)A.browptr, (const int32_t *)A.bcol, (const cplx *)A.blocks, x, y, k, kg,                    \
                           (const int32_t *)A.order);                                                                                   \
    } while (0)
    if (tt > 16) BM(0);
    else if (tt <= 1) BM(1);
    else if (tt <= 2) BM(2);
    else if (tt <= 4) BM(4);
    else if (tt <= 8) BM(8);
    else BM(16);
#undef BM
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

int op_apply_multi_raw(Op *op, const cplx *x, cplx *y, int64_t n, int k, const cplx *w) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    MGCR_CHECK(k >= 1 && k <= MV_MAX_K, MGCR_ERR_INVALID, "k = %d columns, 1 .. %d are supported", k, MV_MAX_K);
    if (n == 0) return MGCR_OK;
    MGCR_CHECK(x != y, MGCR_ERR_INVALID, "the k-wide apply cannot run in place");
    const Op *b0 = op->kind == OP_DIRAC || op->kind == OP_DIRAC_MULTI ? op->base : op;
    MGCR_CHECK(!op->dist && !op->comm && !(b0 && (b0->dist || b0->comm)), MGCR_ERR_UNSUPPORTED,
               "the k-wide apply does not support distributed operators");
    switch (op->kind) {
        case OP_CSR:
            MGCR_CHECK(op->csr.ncol == n, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
            MGCR_CHECK(!w || op->csr.nrow == n, MGCR_ERR_INVALID, "residual form needs a square matrix");
            return w ? csr_apply_multi(op->csr, x, y, k, true, make_double2(1., 0.), nullptr, w)
                     : csr_apply_multi(op->csr, x, y, k, false, make_double2(0., 0.), nullptr, nullptr);
        case OP_DIRAC:
            MGCR_CHECK(!w, MGCR_ERR_INVALID, "residual form: plain Sparse only");
            MGCR_CHECK(b0->kind == OP_CSR && b0->csr.nrow == n && b0->csr.ncol == n, MGCR_ERR_INVALID,
                       "DiracOp needs a square matrix matching the Field dimension");
            MGCR_CHECK(op->k.x != 0. || op->k.y != 0., MGCR_ERR_INVALID, "No k value supplied for Dirac Operator!");
            return csr_apply_multi(b0->csr, x, y, k, true, op->k, nullptr, nullptr);
        case OP_DIRAC_MULTI: {
            MGCR_CHECK(!w, MGCR_ERR_INVALID, "residual form: plain Sparse only");
            MGCR_CHECK(b0->kind == OP_CSR && b0->csr.nrow == n && b0->csr.ncol == n, MGCR_ERR_INVALID,
                       "MultiDiracOp needs a square matrix matching the Field dimension");
            MGCR_CHECK(k == op->nk, MGCR_ERR_INVALID, "MultiDiracOp carries %d hopping parameters, the block has %d columns", op->nk, k);
            KCols ks;
            for (int q = 0; q < MV_MAX_K; q++) ks.v[q] = op->ks[q];   // (entries from k on are 0 and are not read)
            return csr_apply_multi(b0->csr, x, y, k, true, op->ks[0], &ks, nullptr);
        }
        case OP_DIRAC_EO_MULTI:   // the Schur complements on the even half, one k per column (evenodd_multi.hip)
            MGCR_CHECK(!w, MGCR_ERR_INVALID, "residual form: plain Sparse only");
            return eo_apply_multi(op, x, y, n, k);
        case OP_BCSR:
            MGCR_CHECK(!w, MGCR_ERR_INVALID, "residual form: plain Sparse only");
            MGCR_CHECK((int64_t)op->bcsr.nbcol * op->bcsr.bs == n, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
            return bcsr_apply_multi(op->bcsr, x, y, k);
        default:
            set_error("the k-wide apply supports Sparse, DiracOp, MultiDiracOp, MultiEvenOddDiracOp and HierarchicalSparse / Dense operators (not GCR or MG objects)");
            return MGCR_ERR_UNSUPPORTED;
    }
}

}  // namespace mgcr
