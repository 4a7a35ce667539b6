// The device side of the FLEXIBLE batched GCR (gcr_multi.hip: gcr_multi_run with a right preconditioner): what stands between the
// batched outer solve's per-column state (DevState, gcr_dev.h) and a preconditioner that writes a whole block.
//
// A column of the batched solve that has stopped is FROZEN with x updates still pending: m_pending_x_kernel reads them from the
// slots ps[q] when the solve ends.  The preconditioner writes the direction start D_m = M r INTO such a slot, so it may store only
// to the columns that are still active at outer step `it`:
//   gate       one workgroup per column, between the k-wide inner solve's entry and its first apply: column j of the inner solve
//              is cut to 0 steps (both stop words -1, what a clear `active` bit does) when the outer column is frozen, or when the
//              outer solve is about to end on the residual the inner solve was handed — gcr_solve_ends on the fold of the column's
//              |r|^2 partials, close_step's fold and expression and so its bits (the batched form of Gcr32Gate);
//   exit<KC>   y = fp64(x32) as g32m_exit_kernel writes it, stored to the ACTIVE columns only: a frozen column's slot keeps its
//              bits, a column that is gated but still active gets the zeros the single solve gets; the rel bookkeeping is kept;
//   take<KC>   for any other preconditioner, applied k-wide into the block z: the active columns of z into the slot, no arithmetic.
// Streaming kernels with per-column masks.  No kernel reads a word its own launch writes (gate: reads the outer states and partials,
// writes the inner stop words; exit: reads the outer states, writes the inner rel); nothing is exchanged inside a launch, no atomics,
// no waits.
#include <climits>
#include <cmath>

#include "gcr32_state.h"
#include "gcr_dev.h"
#include "multi_dev.h"

namespace mgcr {

// m_active of gcr_multi.hip: the column exists and has not stopped before step `it`
__device__ __forceinline__ bool mflex_active(const DevState *st, int col, int k, int it) {
    return col < k && !(st[col].stop_at < st[col].base + it);
}

__global__ void __launch_bounds__(RED_THREADS) mflex_gate_kernel(const DevState *__restrict__ st, int it, const double *__restrict__ partsR, int nblk,
                                                                 int k, G32Dev *__restrict__ st32) {
    __shared__ double lds[17];
    const int j = (int)blockIdx.x;
    bool cut = !mflex_active(st, j, k, it);   // (uniform over the workgroup)
    if (!cut) {
        double rr[1];
        fold_partials<1>(partsR + (size_t)j * RED_MAX_BLOCKS, nblk, RED_MAX_BLOCKS, rr, lds);
        cut = gcr_solve_ends(rr[0], st[j].bnorm2, st[j].tol2);
    }
    if (cut && threadIdx.x == 0) st32[j].stop_a = st32[j].stop_u = -1;   // 0 steps, x32 = 0 (the entry kernel zeroed it)
}

template <int KC>
__global__ void __launch_bounds__(RED_THREADS) mflex_exit_kernel(const DevState *__restrict__ st, int it, const c32 *__restrict__ x, cplx *__restrict__ y,
                                                                 int64_t nv, int64_t n, int k, const double *__restrict__ S2, int nblkS,
                                                                 G32Dev *__restrict__ st32) {
    __shared__ double lds[2 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) act[c] = mflex_active(st, c0 + c, k, it);
    MV_GRID_STRIDE(i, n) {
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (!act[c]) continue;
            const c32 v = x[(int64_t)(c0 + c) * nv + i];
            y[i * k + c0 + c] = make_double2((double)v.x, (double)v.y);
        }
    }
    if (blockIdx.x == 0) {   // (g32m_exit_kernel's: every column, frozen or not — a cut column's rel is that of 0 steps)
        double s2[2 * KC];
        fold_partials<2 * KC>(S2 + (size_t)2 * c0 * RED_MAX_BLOCKS, nblkS, RED_MAX_BLOCKS, s2, lds);
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (threadIdx.x == 0 && c0 + c < k) st32[c0 + c].rel = s2[2 * c] > 0. ? sqrt(s2[2 * c + 1] / s2[2 * c]) : 0.;
    }
}

template <int KC>
__global__ void __launch_bounds__(256) mflex_take_kernel(const DevState *__restrict__ st, int it, const cplx *__restrict__ z, cplx *__restrict__ slot,
                                                         int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    bool act[KC];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        act[c] = mflex_active(st, c0 + c, k, it);
        any = any || act[c];
    }
    if (!any) return;   // (uniform over the workgroup)
    MV_GRID_STRIDE(i, n) {
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (act[c]) slot[i * k + c0 + c] = z[i * k + c0 + c];
    }
}

// ---- host: the three launches ----------------------------------------------------------------------------------------------------------
template <typename... KA, typename... AA>
static int mflex_launch(void (*kernel)(KA...), dim3 grid, int block, AA... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, ctx().stream, args...);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

int mflex_gate(const MFlexGate &g, int k, G32Dev *st32) {
    return mflex_launch(mflex_gate_kernel, dim3((unsigned)k), RED_THREADS, g.st, g.it, g.partsR, g.nblk, k, st32);
}

int mflex_exit(const MFlexGate &g, const c32 *x, cplx *y, int64_t nv, int64_t n, int k, const double *S2, int nblkS, G32Dev *st32) {
    return dispatch_value<1, 2, 4>(mv_group(k), [&](auto kcc) -> int {
        constexpr int KC = decltype(kcc)::value;
        return mflex_launch(mflex_exit_kernel<KC>, dim3((unsigned)nblkS, (unsigned)((k + KC - 1) / KC)), RED_THREADS, g.st, g.it, x, y, nv, n, k, S2,
                            nblkS, st32);
    });
}

int mflex_take(const DevState *st, int it, const cplx *z, cplx *slot, int64_t n, int k, int blocks) {
    return dispatch_value<1, 2, 4>(mv_group(k), [&](auto kcc) -> int {
        constexpr int KC = decltype(kcc)::value;
        return mflex_launch(mflex_take_kernel<KC>, dim3((unsigned)blocks, (unsigned)((k + KC - 1) / KC)), 256, st, it, z, slot, n, k);
    });
}

}  // namespace mgcr
