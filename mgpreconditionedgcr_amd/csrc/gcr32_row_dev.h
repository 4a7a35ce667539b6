// The ONE row sum of the low-precision GCR's fp32 slabs (device side): g32_apply_kernel (gcr32.hip), the two stages of the even-odd
// form (gcr32_eo.hip) and the k-wide apply (gcr32_multi.hip) call it, so a row is summed the same way wherever its matrix is used.
//   slab   entries 0 .. W - 1 of the row, in stored order, into an accumulator that starts at +0 (padding, column -1, is skipped)
//   tail   a row longer than W: its remaining entries into a SECOND accumulator that starts at +0, which is then added to the first
// Every product is un-fused: real slab (a xr, a xi), complex slab (ar xr - ai xi, ar xi + ai xr).
// g32_row_sum_cols is the per-column form for a block of k interleaved columns (element (row, column) at r[row * k + column]): one
// thread owns the row for K >= k columns, reads every (col, val) once and adds, per column, the same products in the same order.
#pragma once
#include "gcr32_state.h"

namespace mgcr {

// s += a x: the product of one stored entry (ay is not read on a real slab)
template <bool REAL>
__device__ __forceinline__ void g32_add_product(float ax, float ay, c32 xv, float &sx, float &sy) {
    if (REAL) {
        sx += ax * xv.x;
        sy += ax * xv.y;
    } else {
        sx += ax * xv.x - ay * xv.y;
        sy += ax * xv.y + ay * xv.x;
    }
}

// Dirac form: y = own - k32 s, un-fused
__device__ __forceinline__ c32 g32_dirac_shift(c32 k32, c32 own, float sx, float sy) {
    const float kx = k32.x * sx - k32.y * sy, ky = k32.x * sy + k32.y * sx;
    return make_float2(own.x - kx, own.y - ky);
}

template <bool REAL>
__device__ __forceinline__ void g32_row_sum(const G32Mat &A, const c32 *__restrict__ r, int64_t tile, int64_t row, float &sx, float &sy) {
    sx = 0.f;
    sy = 0.f;
    for (int w = 0; w < A.W; w++) {
        const int64_t at = (int64_t)w * A.npad + row;
        const int32_t c = A.col[at];
        if (c < 0) continue;
        const c32 xv = r[c];
        if (REAL) {
            g32_add_product<true>(A.val[at], 0.f, xv, sx, sy);
        } else {
            const c32 a = reinterpret_cast<const c32 *>(A.val)[at];
            g32_add_product<false>(a.x, a.y, xv, sx, sy);
        }
    }
    const int t0 = A.tile_tail[tile], t1 = A.tile_tail[tile + 1];
    for (int t = t0; t < t1; t++) {
        if (A.tail_rows[t] != (int32_t)row) continue;
        float ux = 0.f, uy = 0.f;   // the tail has an accumulator of its own
        for (int e = A.tail_ptr[t]; e < A.tail_ptr[t + 1]; e++) {
            const c32 xv = r[A.tail_col[e]];
            if (REAL) {
                g32_add_product<true>(A.tail_val[e], 0.f, xv, ux, uy);
            } else {
                const c32 a = reinterpret_cast<const c32 *>(A.tail_val)[e];
                g32_add_product<false>(a.x, a.y, xv, ux, uy);
            }
        }
        sx += ux;
        sy += uy;
    }
}

// columns 0 .. k - 1 (k <= K) of the gathered row `c` of a block: 8 k contiguous bytes; the columns beyond k read as 0
template <int K>
__device__ __forceinline__ void g32_gather_cols(const c32 *__restrict__ r, int32_t c, int k, c32 (&xv)[K]) {
    const c32 *xr = r + (int64_t)c * k;
#pragma unroll
    for (int q = 0; q < K; q++) xv[q] = q < k ? xr[q] : make_float2(0.f, 0.f);
}

// The row sum of columns 0 .. k - 1 of a block (k <= K): slab, then the tail's own accumulator, per column.  The slab is touched once
// per apply, so its (col, val) stream is loaded non-temporally.
template <bool REAL, int K>
__device__ __forceinline__ void g32_row_sum_cols(const G32Mat &A, const c32 *__restrict__ r, int k, int64_t tile, int64_t row, float (&sx)[K],
                                                 float (&sy)[K]) {
#pragma unroll
    for (int q = 0; q < K; q++) sx[q] = sy[q] = 0.f;
    for (int w = 0; w < A.W; w++) {
        const int64_t at = (int64_t)w * A.npad + row;
        const int32_t c = __builtin_nontemporal_load(A.col + at);
        if (c < 0) continue;
        c32 xv[K];
        g32_gather_cols<K>(r, c, k, xv);
        float ax, ay = 0.f;
        if (REAL) {
            ax = __builtin_nontemporal_load(A.val + at);
        } else {
            ax = __builtin_nontemporal_load(A.val + 2 * at);
            ay = __builtin_nontemporal_load(A.val + 2 * at + 1);
        }
#pragma unroll
        for (int q = 0; q < K; q++) g32_add_product<REAL>(ax, ay, xv[q], sx[q], sy[q]);
    }
    const int t0 = A.tile_tail[tile], t1 = A.tile_tail[tile + 1];
    for (int t = t0; t < t1; t++) {
        if (A.tail_rows[t] != (int32_t)row) continue;
        float ux[K], uy[K];   // the tail has accumulators of its own
#pragma unroll
        for (int q = 0; q < K; q++) ux[q] = uy[q] = 0.f;
        for (int e = A.tail_ptr[t]; e < A.tail_ptr[t + 1]; e++) {
            c32 xv[K];
            g32_gather_cols<K>(r, A.tail_col[e], k, xv);
            const float ax = REAL ? A.tail_val[e] : A.tail_val[2 * e], ay = REAL ? 0.f : A.tail_val[2 * e + 1];
#pragma unroll
            for (int q = 0; q < K; q++) g32_add_product<REAL>(ax, ay, xv[q], ux[q], uy[q]);
        }
#pragma unroll
        for (int q = 0; q < K; q++) {
            sx[q] += ux[q];
            sy[q] += uy[q];
        }
    }
}

}  // namespace mgcr
