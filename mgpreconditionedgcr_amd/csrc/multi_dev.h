// Device-side helpers shared by the multi-vector kernels (mvec.hip, spmm.hip, gcr_multi.hip).
//
// A multi-vector holds k Fields with the columns interleaved: element (row i, column j) at d[i * k + j].  The streaming
// kernels (BLAS-1, the batched GCR's updates) deal the ROWS to threads exactly as the single-Field kernels do — grid of
// red_grid(n) workgroups of RED_THREADS threads, grid-stride — and a thread carries KC <= 4 neighbouring columns of its
// rows (a 64-byte piece of the row); gridDim.y = ceil(k / KC) column groups.  Per column a thread therefore adds the same
// rows in the same order as the single kernel's thread, and block_sum_owner builds the same tree per scalar whatever the
// number of scalars that share its exchanges (reduce.h): column j's partial sums have the bits of the single kernel's.
#pragma once
#include "internal.h"
#include "reduce.h"

namespace mgcr {

#define MV_GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// The shift of the k-wide apply (spmm.hip): one k for all columns, or one k per column.  KCols is passed BY VALUE in the kernel
// arguments: a launch keeps the values it was enqueued with whatever mgcr_dirac_multi_set_k does afterwards, and a thread reads
// them as scalars.
struct KUniform {
    cplx k;
    __device__ __forceinline__ cplx at(int) const { return k; }
};
struct KCols {
    cplx v[MV_MAX_K];
    __device__ __forceinline__ cplx at(int q) const { return v[q]; }
};

// columns per thread of the streaming kernels
inline int mv_group(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : 4; }

// columns [c0, c0 + KC) of row i; columns >= k read as 0
template <int KC>
__device__ __forceinline__ void mv_load(const cplx *p, int64_t i, int k, int c0, cplx (&v)[KC]) {
#pragma unroll
    for (int c = 0; c < KC; c++) v[c] = c0 + c < k ? p[i * k + c0 + c] : make_double2(0., 0.);
}

}  // namespace mgcr
