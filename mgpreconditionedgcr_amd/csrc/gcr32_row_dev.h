// The ONE row sum of the low-precision GCR's fp32 slabs (device side): g32_apply_kernel (gcr32.hip) and the two stages of the even-odd
// form (gcr32_eo.hip) call it, so a row is summed the same way wherever its matrix is used.
//   slab   entries 0 .. W - 1 of the row, in stored order, into an accumulator that starts at +0 (padding, column -1, is skipped)
//   tail   a row longer than W: its remaining entries into a SECOND accumulator that starts at +0, which is then added to the first
// Every product is un-fused: real slab (a xr, a xi), complex slab (ar xr - ai xi, ar xi + ai xr).
#pragma once
#include "gcr32_state.h"

namespace mgcr {

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
            const float a = A.val[at];
            sx += a * xv.x;
            sy += a * xv.y;
        } else {
            const c32 a = reinterpret_cast<const c32 *>(A.val)[at];
            sx += a.x * xv.x - a.y * xv.y;
            sy += a.x * xv.y + a.y * xv.x;
        }
    }
    const int t0 = A.tile_tail[tile], t1 = A.tile_tail[tile + 1];
    for (int t = t0; t < t1; t++) {
        if (A.tail_rows[t] != (int32_t)row) continue;
        float ux = 0.f, uy = 0.f;   // the tail has an accumulator of its own
        for (int e = A.tail_ptr[t]; e < A.tail_ptr[t + 1]; e++) {
            const c32 xv = r[A.tail_col[e]];
            if (REAL) {
                const float a = A.tail_val[e];
                ux += a * xv.x;
                uy += a * xv.y;
            } else {
                const c32 a = reinterpret_cast<const c32 *>(A.tail_val)[e];
                ux += a.x * xv.x - a.y * xv.y;
                uy += a.x * xv.y + a.y * xv.x;
            }
        }
        sx += ux;
        sy += uy;
    }
}

}  // namespace mgcr
