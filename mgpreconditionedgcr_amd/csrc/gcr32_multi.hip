// The low-precision GCR on a block of k Fields: the k inner solves of mgcr_gcr32_apply_multi advance in LOCKSTEP and share every
// launch, so the fp32 slab is streamed once per step for all k columns; and the batched mixed solve mgcr_gcr32_solve_multi, fp64
// defect correction around it (include/mgcr.h has the rules, DESIGN.md §11.2 the byte model and the measurements).
//
// Rule M1: column j of the result, its step count and its rel_res are BIT-IDENTICAL to the single apply (gcr32.hip) on column j.
// Per column every kernel below keeps the single kernels' row-to-thread map, grid, block_sum_owner / fold_partials trees (reduce.h:
// a scalar's tree does not depend on the scalars that share its exchanges) and calls their element-wise expressions
// (gcr32_elem_dev.h, gcr32_row_dev.h).
//
// Layout.  F and Y are blocks with the columns interleaved, element (row, column) at [row * k + column].  The operator's own vectors
// (r, Ar, x, the slots) are PLANAR, column c of a vector at [c * nv, c * nv + n): a column is laid out as the single solve's vector, so
// the streaming kernels run the single kernels' 16-byte coalesced accesses with blockIdx.y = the column.  (The first version kept
// them interleaved, 4 columns per thread: a lane then touched 32 bytes at a stride of 8 k, and build + update + dots took 2.8 ms of
// a 3.55 ms lockstep step at k = 12 on the 16^4 x 12 lattice, eight times the twelve single kernels.)  Only the apply's gather wants
// a row's k values side by side: r is kept a second time interleaved (rg), written by the entry and update kernels.
//
//   entry<KC>      r, rg = fp32(F), x = 0, the partials of |f_j|^2, the k states reset (a column whose `active` bit is clear: stopped)
//   step it  apply<K, REAL>   per column the stop test on the folded |r|^2 and |f|^2; Ar = A32 rg, one thread per row for all columns
//            dots<ND>         the partials of <Ap_i, Ar>, i < ND, with the single apply's tile map (not launched for ND = 0)
//            build<ND>        fold, beta_i, p and Ap into slot ND, the partials of <Ap, Ap> and <Ap, r>
//            update           fold, alpha, x, r, rg, the partials of |r|^2, the step counter
//   exit<KC>       Y = fp64(x), |r| / |f| per column
// dots, build and update: gridDim.y = k, one column per workgroup row; entry and exit, which read and write the interleaved blocks:
// KC = mv_group(k) columns per thread, gridDim.y column groups.  max_iter steps are enqueued whatever the data: 4 launches per step,
// 3 for the step that opens a restart cycle, plus entry and exit.
//
// Per-column state: one G32Dev per column and per-column partial slabs ([column][scalar][RED_MAX_BLOCKS]).  The per-column scalars
// are folded in every workgroup's prologue, as in gcr32.hip (a scalar kernel per phase would add three launches to a step that is
// launch-bound on the small operators): a workgroup of the streaming kernels folds its own column's, the apply ceil(k / 4) folds of
// four columns each, from cache-resident slabs.  A column that has stopped is FROZEN: its stop words say so to every later kernel,
// which neither folds for it nor stores to it.  As in gcr32.hip no kernel reads a word its own launch writes (apply: reads stop_u,
// writes stop_a; update: reads stop_a, writes stop_u; dots and build read both), nothing is exchanged inside a launch, no atomics,
// no waits.
#include <climits>
#include <cmath>

#include "gcr32_elem_dev.h"
#include "gcr32_row_dev.h"
#include "gcr32_state.h"
#include "multi_dev.h"

namespace mgcr {

constexpr int G32M_PB = 2 * GCR32_MAX_RESTART;   // scalars per column of the <Ap_i, Ar> slab

struct Gcr32MultiState {
    int k = 0, restart = 0;
    c32 *r = nullptr, *ar = nullptr, *x = nullptr, *ps = nullptr, *aps = nullptr;   // [k][nv] planar; ps, aps: restart slots of that
    c32 *rg = nullptr;          // r once more, [nv][k] interleaved: what the apply gathers from
    double *S2 = nullptr;       // [MV_MAX_K][2][RED_MAX_BLOCKS]: |f|^2, |r|^2
    double *partsA = nullptr;   // [MV_MAX_K][3][RED_MAX_BLOCKS]: <Ap, Ap>, <Ap, r>
    double *partsB = nullptr;   // [MV_MAX_K][G32M_PB][RED_MAX_BLOCKS]: <Ap_i, Ar>
    G32Dev *st = nullptr;       // [MV_MAX_K]
    // the work blocks of mgcr_gcr32_solve_multi: kept while n and k stay
    int wk_k = 0;
    cplx *R = nullptr, *E = nullptr, *AX = nullptr;
};

static int64_t g_multi_applies = 0, g_multi_steps = 0;   // enqueued; under the context's lock
int64_t gcr32_multi_stat(int which) { return which == 0 ? g_multi_applies : g_multi_steps; }

// bit c: column c0 + c exists and neither stop word says it ended before step `it` (use_a / use_u: the words this kernel may read)
template <int KC>
__device__ __forceinline__ unsigned g32m_running(const G32Dev *__restrict__ st, int c0, int k, int it, bool use_a, bool use_u) {
    unsigned on = 0;
#pragma unroll
    for (int c = 0; c < KC; c++) {
        if (c0 + c >= k) continue;
        if (use_a && st[c0 + c].stop_a < it) continue;
        if (use_u && st[c0 + c].stop_u < it) continue;
        on |= 1u << c;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)on);
}

// ---- entry ------------------------------------------------------------------------------------------------------------------------
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) g32m_entry_kernel(const cplx *__restrict__ f, c32 *__restrict__ r, c32 *__restrict__ rg, c32 *__restrict__ x,
                                                                 int64_t nv, int64_t n, int k, unsigned active, G32Dev *__restrict__ st,
                                                                 double *__restrict__ S2) {
    __shared__ double lds[KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    if (blockIdx.x == 0 && (int)threadIdx.x < KC && c0 + (int)threadIdx.x < k) {
        G32Dev *s = st + c0 + threadIdx.x;
        s->stop_a = s->stop_u = ((active >> (c0 + threadIdx.x)) & 1u) ? INT_MAX : -1;   // -1: 0 steps, y = 0
        s->n_iter = 0;
        s->rel = 0.;
    }
    double acc[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) acc[c] = 0.;
    const int64_t npair = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (c0 + c >= k) continue;
            const int64_t e0 = 2 * i * k + c0 + c, e1 = e0 + k;
            const cplx a = f[e0], b = f[e1];
            const float4 v = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
            rg[e0] = make_float2(v.x, v.y);
            rg[e1] = make_float2(v.z, v.w);
            reinterpret_cast<float4 *>(r + (int64_t)(c0 + c) * nv)[i] = v;
            reinterpret_cast<float4 *>(x + (int64_t)(c0 + c) * nv)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            acc[c] += norm2d(v.x, v.y);
            acc[c] += norm2d(v.z, v.w);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (c0 + c >= k) continue;
            const cplx a = f[(n - 1) * k + c0 + c];
            const c32 v = make_float2((float)a.x, (float)a.y);
            rg[(n - 1) * k + c0 + c] = v;
            r[(int64_t)(c0 + c) * nv + n - 1] = v;
            x[(int64_t)(c0 + c) * nv + n - 1] = make_float2(0.f, 0.f);
            acc[c] += norm2d(v.x, v.y);
        }
    }
    const double mine = block_sum_owner<KC>(acc, lds);
    if ((int)threadIdx.x < KC && c0 + (int)threadIdx.x < k) {
        double *s = S2 + (size_t)(c0 + threadIdx.x) * 2 * RED_MAX_BLOCKS + blockIdx.x;
        s[0] = mine;
        s[RED_MAX_BLOCKS] = mine;
    }
}

// ---- apply: Ar = A32 r, one thread per row for all K >= k columns -------------------------------------------------------------------
template <int K, bool REAL>
__global__ void __launch_bounds__(RED_THREADS, 4)
    g32m_apply_kernel(G32Mat A, const c32 *__restrict__ rg, c32 *__restrict__ ar, int64_t nv, int64_t n, int k, int dirac, c32 k32,
                      const double *__restrict__ S2, int nblkS, double tol2, G32Dev *__restrict__ st, int it) {
    __shared__ double lds[8 * 17];
    unsigned live = 0;
    for (int c0 = 0; c0 < k; c0 += 4) {   // four columns' |f|^2 and |r|^2 per fold
        const unsigned on = g32m_running<4>(st, c0, k, it, false, true);
        if (!on) continue;
        double s2[8];
        fold_partials<8>(S2 + (size_t)c0 * 2 * RED_MAX_BLOCKS, nblkS, RED_MAX_BLOCKS, s2, lds);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (!((on >> c) & 1u)) continue;
            if (!(s2[2 * c + 1] > tol2 * s2[2 * c])) {   // |r|^2 <= tol^2 |f|^2, f = 0 included: the column's solve is over with what x holds
                if (blockIdx.x == 0 && threadIdx.x == 0) st[c0 + c].stop_a = it - 1;
                continue;
            }
            live |= 1u << (c0 + c);
        }
    }
    live = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
    if (!live) return;
    const int64_t ntiles = (n + G32_TILE - 1) / G32_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * G32_TILE + threadIdx.x;
        if (row < n) {
            float sx[K], sy[K];
            g32_row_sum_cols<REAL, K>(A, rg, k, tile, row, sx, sy);
#pragma unroll
            for (int q = 0; q < K; q++) {
                if (!((live >> q) & 1u)) continue;
                c32 y = make_float2(sx[q], sy[q]);
                if (dirac) y = g32_dirac_shift(k32, rg[row * k + q], sx[q], sy[q]);
                ar[(int64_t)q * nv + row] = y;   // planar: a wave stores 512 contiguous bytes per column
            }
        }
    }
}

// ---- dots: the partials of <Ap_i, Ar>, i < ND, with the single apply's map (tile = blockIdx.x + m gridDim.x, row = tile * 1024 + thread) ----
// NC <= 8 directions of one column, 16 scalars: one chunk of block_sums_to_slab (a scalar's tree does not depend on the chunking)
template <int NC>
__device__ __forceinline__ void g32m_dots_body(const c32 *__restrict__ ar, const c32 *__restrict__ aps, int64_t slot, int64_t n,
                                               double *__restrict__ partsB, double *lds) {
    double acc[2 * NC];
#pragma unroll
    for (int s = 0; s < 2 * NC; s++) acc[s] = 0.;
    const int64_t ntiles = (n + G32_TILE - 1) / G32_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row = tile * G32_TILE + threadIdx.x;
        if (row < n) {
            const c32 y = ar[row];
            const double yx = (double)y.x, yy = (double)y.y;
            const c32 *pa = aps + row;   // one running pointer walks the slots
#pragma unroll
            for (int j = 0; j < NC; j++) {   // <Ap_j, Ar> = sum conj(Ap_j) Ar
                const c32 a = *pa;
                pa += slot;
                g32_beta_dot(a.x, a.y, yx, yy, acc[2 * j], acc[2 * j + 1]);
            }
        }
    }
    block_sums_to_slab<2 * NC>(acc, lds, partsB, blockIdx.x);
}
// blockIdx.y: the column.  gridDim.z = 1 (ND <= 8) or 2: 30 double accumulators beside the loads do not fit 128 registers, so the
// workgroups z = 0 take the first 8 directions and z = 1 the other ND - 8 (Ar is read twice then)
template <int ND>
__global__ void __launch_bounds__(RED_THREADS, 4)
    g32m_dots_kernel(const c32 *__restrict__ ar, const c32 *__restrict__ aps, int64_t nv, int64_t slot, int64_t n, int k, const G32Dev *__restrict__ st,
                     int it, double *__restrict__ partsB) {
    constexpr int N0 = ND < 8 ? ND : 8;
    __shared__ double lds[2 * N0 * 17];
    const int c = (int)blockIdx.y;
    if (!g32m_running<1>(st, c, k, it, true, true)) return;
    ar += (int64_t)c * nv;
    aps += (int64_t)c * nv;
    partsB += (size_t)c * G32M_PB * RED_MAX_BLOCKS;
    if constexpr (ND > 8) {
        if (blockIdx.z == 1) {
            g32m_dots_body<ND - 8>(ar, aps + 8 * slot, slot, n, partsB + (size_t)16 * RED_MAX_BLOCKS, lds);
            return;
        }
    }
    g32m_dots_body<N0>(ar, aps, slot, n, partsB, lds);
}

// ---- build: beta_i, p = r - sum beta_i p_i and Ap = Ar - sum beta_i Ap_i into slot ND, <Ap, Ap> and <Ap, r> (blockIdx.y: the column) ----
template <int ND>
__global__ void __launch_bounds__(RED_THREADS, (ND <= 5 ? 8 : 4))
    g32m_build_kernel(const float *__restrict__ r, const float *__restrict__ ar, float *__restrict__ ps, float *__restrict__ aps, int64_t nv, int64_t slot,
                      int64_t n, int k, const double *__restrict__ partsB, int nblkB, G32Dev *__restrict__ st, int it, double *__restrict__ partsA) {
    const int c = (int)blockIdx.y;
    if (!g32m_running<1>(st, c, k, it, true, true)) return;
    __shared__ double lds[(2 * ND > 16 ? 16 : 2 * ND > 3 ? 2 * ND : 3) * 17];
    __shared__ float beta[ND ? 2 * ND : 2];
    if constexpr (ND > 0) {
        fold_betas<ND>(partsB + (size_t)c * G32M_PB * RED_MAX_BLOCKS, nblkB, st[c].den, beta, lds);
        __syncthreads();
    }
    r += 2 * c * nv;
    ar += 2 * c * nv;
    ps += 2 * c * nv;
    aps += 2 * c * nv;
    double acc[3] = {0., 0., 0.};
    const int64_t npair = n >> 1, half = slot >> 1;   // (slot: c32 elements between two slots of one column; nv is a multiple of 4)
    const float4 *r4 = reinterpret_cast<const float4 *>(r), *ar4 = reinterpret_cast<const float4 *>(ar);
    float4 *ps4 = reinterpret_cast<float4 *>(ps), *aps4 = reinterpret_cast<float4 *>(aps);
    for (int64_t b0 = (int64_t)blockIdx.x * RED_THREADS; b0 < npair; b0 += (int64_t)gridDim.x * RED_THREADS) {
        const unsigned t = threadIdx.x;
        if (b0 + t >= npair) break;
        const float4 rr = (r4 + b0)[t];
        float4 p = rr, q = (ar4 + b0)[t];
        float4 *pp = ps4 + b0 + t, *qq = aps4 + b0 + t;   // two running pointers walk the slots, two directions' loads in flight
#pragma unroll 2
        for (int j = 0; j < ND; j++) {
            const float4 pj = *pp, qj = *qq;
            const float bx = beta[2 * j], by = beta[2 * j + 1];
            pp += half;
            qq += half;
            g32_sub_scaled(bx, by, pj.x, pj.y, p.x, p.y);
            g32_sub_scaled(bx, by, pj.z, pj.w, p.z, p.w);
            g32_sub_scaled(bx, by, qj.x, qj.y, q.x, q.y);
            g32_sub_scaled(bx, by, qj.z, qj.w, q.z, q.w);
        }
        g32_build_dots(q.x, q.y, rr.x, rr.y, acc);
        g32_build_dots(q.z, q.w, rr.z, rr.w, acc);
        *pp = p;      // slot ND
        *qq = q;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
        const int64_t e = n - 1;
        const c32 rr = reinterpret_cast<const c32 *>(r)[e];
        c32 p = rr, q = reinterpret_cast<const c32 *>(ar)[e];
        for (int j = 0; j < ND; j++) {
            const c32 pj = reinterpret_cast<const c32 *>(ps)[(int64_t)j * slot + e], qj = reinterpret_cast<const c32 *>(aps)[(int64_t)j * slot + e];
            g32_sub_scaled(beta[2 * j], beta[2 * j + 1], pj.x, pj.y, p.x, p.y);
            g32_sub_scaled(beta[2 * j], beta[2 * j + 1], qj.x, qj.y, q.x, q.y);
        }
        g32_build_dots(q.x, q.y, rr.x, rr.y, acc);
        reinterpret_cast<c32 *>(ps)[(int64_t)ND * slot + e] = p;
        reinterpret_cast<c32 *>(aps)[(int64_t)ND * slot + e] = q;
    }
    block_sums_to_slab<3>(acc, lds, partsA + (size_t)3 * c * RED_MAX_BLOCKS, blockIdx.x);
}

// ---- update: alpha, x += alpha p, r -= alpha Ap (both copies of r), |r|^2, the step counter (blockIdx.y: the column) ----------------------
__global__ void __launch_bounds__(RED_THREADS, 8)
    g32m_update_kernel(float *__restrict__ x, float *__restrict__ r, c32 *__restrict__ rg, const float *__restrict__ p, const float *__restrict__ ap, int64_t nv,
                       int64_t n, int k, const double *__restrict__ partsA, int nblkA, G32Dev *__restrict__ st, int it, int slot, double *__restrict__ S2) {
    const int c = (int)blockIdx.y;
    if (!g32m_running<1>(st, c, k, it, true, false)) return;
    __shared__ double lds[3 * 17];
    double v[3];
    fold_partials<3>(partsA + (size_t)3 * c * RED_MAX_BLOCKS, nblkA, RED_MAX_BLOCKS, v, lds);
    if (!(v[0] > 0.)) {   // <Ap, Ap> exactly zero: the column's solve is over with what x holds
        if (blockIdx.x == 0 && threadIdx.x == 0) st[c].stop_u = it - 1;
        return;
    }
    const float ax = uniform((float)(v[1] / v[0])), ay = uniform((float)(v[2] / v[0]));   // formed in fp64, rounded once
    x += 2 * c * nv;
    r += 2 * c * nv;
    p += 2 * c * nv;
    ap += 2 * c * nv;
    rg += c;
    double acc[1] = {0.};
    const int64_t npair = n >> 1;
    float4 *x4 = reinterpret_cast<float4 *>(x), *r4 = reinterpret_cast<float4 *>(r);
    const float4 *p4 = reinterpret_cast<const float4 *>(p), *q4 = reinterpret_cast<const float4 *>(ap);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
        float4 xv = x4[i], rv = r4[i];
        const float4 pv = p4[i], qv = q4[i];
        g32_update_one(ax, ay, pv.x, pv.y, qv.x, qv.y, xv.x, xv.y, rv.x, rv.y, acc[0]);
        g32_update_one(ax, ay, pv.z, pv.w, qv.z, qv.w, xv.z, xv.w, rv.z, rv.w, acc[0]);
        x4[i] = xv;
        r4[i] = rv;
        rg[2 * i * k] = make_float2(rv.x, rv.y);   // the apply's copy
        rg[(2 * i + 1) * k] = make_float2(rv.z, rv.w);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last element
        const int64_t e = n - 1;
        c32 xv = reinterpret_cast<c32 *>(x)[e], rv = reinterpret_cast<c32 *>(r)[e];
        const c32 pv = reinterpret_cast<const c32 *>(p)[e], qv = reinterpret_cast<const c32 *>(ap)[e];
        g32_update_one(ax, ay, pv.x, pv.y, qv.x, qv.y, xv.x, xv.y, rv.x, rv.y, acc[0]);
        reinterpret_cast<c32 *>(x)[e] = xv;
        reinterpret_cast<c32 *>(r)[e] = rv;
        rg[e * k] = rv;
    }
    const double mine = block_sum_owner<1>(acc, lds);
    if (threadIdx.x == 0) S2[(size_t)c * 2 * RED_MAX_BLOCKS + RED_MAX_BLOCKS + blockIdx.x] = mine;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st[c].n_iter = it; st[c].den[slot] = v[0]; }
}

// ---- exit: Y = fp64(x), |r| / |f| behind each column's last step -----------------------------------------------------------------------
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) g32m_exit_kernel(const c32 *__restrict__ x, cplx *__restrict__ y, int64_t nv, int64_t n, int k,
                                                                const double *__restrict__ S2, int nblkS, G32Dev *__restrict__ st) {
    __shared__ double lds[2 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    MV_GRID_STRIDE(i, n) {
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (c0 + c >= k) continue;
            const c32 v = x[(int64_t)(c0 + c) * nv + i];
            y[i * k + c0 + c] = make_double2((double)v.x, (double)v.y);
        }
    }
    if (blockIdx.x == 0) {
        double s2[2 * KC];
        fold_partials<2 * KC>(S2 + (size_t)2 * c0 * RED_MAX_BLOCKS, nblkS, RED_MAX_BLOCKS, s2, lds);
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (threadIdx.x == 0 && c0 + c < k) st[c0 + c].rel = s2[2 * c] > 0. ? sqrt(s2[2 * c + 1] / s2[2 * c]) : 0.;
    }
}

// ---- the defect correction's block kernels: mgcr_axpy(1, e, x) and mgcr_add_scaled(r, b, -1, t) per column ------------------------------
// x_j = x_j + 1 e_j on the columns of `mask`, the arithmetic of add_scaled_kernel (blas1.hip); every other column keeps its bits
// (a thread owns a row's k neighbouring values: no division to find the column)
__global__ void __launch_bounds__(RED_THREADS) g32m_correct_kernel(cplx *__restrict__ x, const cplx *__restrict__ e, int64_t n, int k, unsigned mask) {
    MV_GRID_STRIDE(i, n) {
        for (int c = 0; c < k; c++)
            if ((mask >> c) & 1u) x[i * k + c] = cadd(x[i * k + c], cmul(make_double2(1., 0.), e[i * k + c]));
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static void g32m_free_vectors(Gcr32MultiState *m) {
    hipFree(m->r); hipFree(m->rg); hipFree(m->ar); hipFree(m->x); hipFree(m->ps); hipFree(m->aps);
    m->r = m->rg = m->ar = m->x = m->ps = m->aps = nullptr;
    m->k = m->restart = 0;
}
static void g32m_free_work(Gcr32MultiState *m) {
    hipFree(m->R); hipFree(m->E); hipFree(m->AX);
    m->R = m->E = m->AX = nullptr;
    m->wk_k = 0;
}
void gcr32_multi_destroy(Gcr32MultiState *m) {
    if (!m) return;
    g32m_free_vectors(m);
    g32m_free_work(m);
    hipFree(m->S2); hipFree(m->partsA); hipFree(m->partsB); hipFree(m->st);
    delete m;
}

template <typename T>
static int g32m_zeroed(T **p, size_t count) {
    MGCR_TRY(g32_alloc(p, count));
    if (hipMemsetAsync(*p, 0, sizeof(T) * count, ctx().stream) != hipSuccess) {
        hipFree(*p);
        *p = nullptr;
        set_error("hipMemsetAsync of the batched low-precision GCR's slabs failed");
        return MGCR_ERR_HIP;
    }
    return MGCR_OK;
}

// r (twice: planar and interleaved), Ar, x and 2 * restart slot blocks of nv * k float2, the slabs and the states: made at the first batched apply of width k, made
// again (behind a stream synchronisation: nothing queued may still use the old ones) when k or restart changes
static int g32m_storage(Gcr32State *g, int k) {
    if (!g->mw) g->mw = new Gcr32MultiState();
    Gcr32MultiState *m = g->mw;
    // (each made once: a failed allocation leaves the ones before it in place for the next call, and for gcr32_multi_destroy)
    if (!m->S2) { MGCR_TRY(g32m_zeroed(&m->S2, (size_t)MV_MAX_K * 2 * RED_MAX_BLOCKS)); }
    if (!m->partsA) { MGCR_TRY(g32m_zeroed(&m->partsA, (size_t)MV_MAX_K * 3 * RED_MAX_BLOCKS)); }
    if (!m->partsB) { MGCR_TRY(g32m_zeroed(&m->partsB, (size_t)MV_MAX_K * G32M_PB * RED_MAX_BLOCKS)); }
    if (!m->st) { MGCR_TRY(g32m_zeroed(&m->st, (size_t)MV_MAX_K)); }
    if (m->k == k && m->restart == g->restart) return MGCR_OK;
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    g32m_free_vectors(m);
    const size_t ne = (size_t)g->nv * k;
    int rc = g32_alloc(&m->r, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->rg, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->ar, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->x, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->ps, ne * g->restart);
    if (rc == MGCR_OK) rc = g32_alloc(&m->aps, ne * g->restart);
    if (rc != MGCR_OK) { g32m_free_vectors(m); return rc; }
    m->k = k;
    m->restart = g->restart;
    return MGCR_OK;
}

static G32Mat g32m_mat(const Gcr32State *g) {
    return G32Mat{g->val, g->col, g->npad, g->W, g->tile_tail, g->tail_rows, g->tail_ptr, g->tail_col, g->tail_val};
}

// f(integral_constant<int, KC>) with KC = min(mv_group(k), cap), cap one of 1, 2, 4 (entry and exit: columns per thread)
template <typename F>
static int g32m_dispatch_kc(int k, int cap, F &&f) {
    const int kc = mv_group(k) < cap ? mv_group(k) : cap;
    if (kc == 1) return f(std::integral_constant<int, 1>{});
    if (kc == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}
template <typename... KA, typename... AA>
static int g32m_launch(void (*kernel)(KA...), int gx, int gy, int gz, AA... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(RED_THREADS), 0, ctx().stream, args...);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

// gate != nullptr (the flexible batched solve, gcr_multi.hip): behind the entry kernel one launch cuts the columns that the outer solve
// has frozen or is about to end on, and the exit stores to the outer solve's active columns only (gcr_multi_flex.hip).  Without it
// every launch is what it was.
static int gcr32_apply_multi(Gcr32State *g, const cplx *f, cplx *y, int k, unsigned active, const MFlexGate *gate = nullptr) {
    MGCR_TRY(g32m_storage(g, k));
    Gcr32MultiState *m = g->mw;
    const int64_t n = g->n, nv = g->nv, slot = g->nv * k;
    const int ga = red_grid(n), gs = red_grid(n >> 1);
    const double tol2 = g->tol * g->tol;
    constexpr int MAX_ND = GCR32_MAX_RESTART - 1;
    g_multi_applies += 1;
    g_multi_steps += g->max_iter;
    const int erc = g32m_dispatch_kc(k, 4, [&](auto kcc) {
        constexpr int KC = decltype(kcc)::value;
        return g32m_launch(g32m_entry_kernel<KC>, gs, (k + KC - 1) / KC, 1, f, m->r, m->rg, m->x, nv, n, k, active, m->st, m->S2);
    });
    MGCR_TRY(erc);
    if (gate) MGCR_TRY(mflex_gate(*gate, k, m->st));
    const int K = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
    for (int it = 1; it <= g->max_iter; it++) {
        const int nd = (it - 1) % g->restart;   // directions stored when the step starts; the new one goes into slot nd
        const int arc = dispatch_bool(g->real, [&](auto real) {
            return dispatch_value<1, 2, 4, 8, 16>(K, [&](auto kc) {
                return launch(g32m_apply_kernel<decltype(kc)::value, decltype(real)::value>, ga, RED_THREADS, 0, g32m_mat(g), (const c32 *)m->rg, m->ar, nv, n, k,
                              g->dirac ? 1 : 0, g->k32, (const double *)m->S2, gs, tol2, m->st, it);
            });
        });
        MGCR_TRY(arc);
        if (nd > 0) {
            const int drc = dispatch_nd<1, MAX_ND>(nd, [&](auto ndc) {
                constexpr int ND = decltype(ndc)::value;
                return g32m_launch(g32m_dots_kernel<ND>, ga, k, ND > 8 ? 2 : 1, (const c32 *)m->ar, (const c32 *)m->aps, nv, slot, n, k, (const G32Dev *)m->st, it,
                                   m->partsB);
            });
            MGCR_TRY(drc);
        }
        const int brc = dispatch_nd<0, MAX_ND>(nd, [&](auto ndc) {
            return g32m_launch(g32m_build_kernel<decltype(ndc)::value>, gs, k, 1, (const float *)m->r, (const float *)m->ar, (float *)m->ps, (float *)m->aps, nv, slot, n,
                               k, (const double *)m->partsB, ga, m->st, it, m->partsA);
        });
        MGCR_TRY(brc);
        MGCR_TRY(g32m_launch(g32m_update_kernel, gs, k, 1, (float *)m->x, (float *)m->r, m->rg, (const float *)(m->ps + (size_t)slot * nd),
                             (const float *)(m->aps + (size_t)slot * nd), nv, n, k, (const double *)m->partsA, gs, m->st, it, nd, m->S2));
    }
    if (gate) return mflex_exit(*gate, (const c32 *)m->x, y, nv, n, k, (const double *)m->S2, gs, m->st);
    return g32m_dispatch_kc(k, 4, [&](auto kcc) {
        constexpr int KC = decltype(kcc)::value;
        return g32m_launch(g32m_exit_kernel<KC>, gs, (k + KC - 1) / KC, 1, (const c32 *)m->x, y, nv, n, k, (const double *)m->S2, gs, m->st);
    });
}

// what the right_precond slot of the flexible batched solve (mgcr_gcr_solve_multi on n rows) asks of a low-precision GCR; k is not
// compared (gcr32_slot_check: a preconditioner at another k is legitimate)
int gcr32_multi_slot_check(const Op *low, int64_t n, const char *who) {
    MGCR_CHECK(low->g32 && !low->g32->eo, MGCR_ERR_UNSUPPORTED, "%s: the even-odd form of the low-precision GCR has no batched inner solve", who);
    MGCR_CHECK(low->g32->n == n, MGCR_ERR_INVALID, "%s: the low-precision GCR has %lld rows, the operator of the solve %lld", who, (long long)low->g32->n,
               (long long)n);
    return MGCR_OK;
}

int gcr32_apply_multi_raw(Op *low, const cplx *f, cplx *y, int64_t n, int k, const MFlexGate *gate) {
    Gcr32State *g = low->g32;
    MGCR_CHECK(g->n == n, MGCR_ERR_INVALID, "low-precision GCR of %lld rows applied to a block of %lld rows", (long long)g->n, (long long)n);
    return gcr32_apply_multi(g, f, y, k, (1u << k) - 1u, gate);   // (k <= MV_MAX_K = 16)
}

static int g32m_work(Gcr32State *g, int k) {
    if (!g->mw) g->mw = new Gcr32MultiState();
    Gcr32MultiState *m = g->mw;
    if (m->wk_k == k) return MGCR_OK;
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    g32m_free_work(m);
    const size_t ne = (size_t)(g->n ? g->n : 1) * k;
    int rc = g32_alloc(&m->R, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->E, ne);
    if (rc == MGCR_OK) rc = g32_alloc(&m->AX, ne);
    if (rc != MGCR_OK) { g32m_free_work(m); return rc; }
    m->wk_k = k;
    return MGCR_OK;
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

// what both entry points ask of `low`
static int g32m_check_low(mgcr_op_t low, const char *who) {
    MGCR_CHECK(low && low->kind == OP_GCR32 && low->g32, MGCR_ERR_INVALID, "%s: not a low-precision GCR", who);
    MGCR_CHECK(!low->g32->eo, MGCR_ERR_UNSUPPORTED, "%s: the even-odd form of the low-precision GCR has no batched inner solve", who);
    return MGCR_OK;
}

extern "C" {

int mgcr_gcr32_apply_multi(mgcr_op_t low, mgcr_mvec_t F, mgcr_mvec_t Y, uint32_t active) {
    const char *who = "mgcr_gcr32_apply_multi";
    MGCR_TRY(require_ctx());
    MGCR_TRY(g32m_check_low(low, who));
    MGCR_CHECK(F && Y, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_CHECK(F->n == Y->n && F->k == Y->k, MGCR_ERR_INVALID, "%s: F is %lld x %d, Y is %lld x %d", who, (long long)F->n, (int)F->k, (long long)Y->n,
               (int)Y->k);
    MGCR_CHECK(F->n == low->g32->n, MGCR_ERR_INVALID, "%s: low-precision GCR of %lld rows applied to a block of %lld rows", who, (long long)low->g32->n,
               (long long)F->n);
    MGCR_CHECK(F->k >= 1 && F->k <= MV_MAX_K, MGCR_ERR_INVALID, "%s: k = %d columns, 1 .. %d are supported", who, (int)F->k, MV_MAX_K);
    MGCR_CHECK((active >> F->k) == 0, MGCR_ERR_INVALID, "%s: active = 0x%x has bits at or above k = %d", who, (unsigned)active, (int)F->k);
    MGCR_CHECK(F != Y && (F->d != Y->d || !F->d), MGCR_ERR_INVALID, "%s: input and output must be different blocks", who);
    if (F->n == 0) return MGCR_OK;
    LOCK();
    return gcr32_apply_multi(low->g32, F->d, Y->d, F->k, active);
}

int mgcr_gcr32_last_multi(mgcr_op_t low, int32_t *n_iter, double *rel_res) {
    const char *who = "mgcr_gcr32_last_multi";
    MGCR_TRY(require_ctx());
    MGCR_TRY(g32m_check_low(low, who));
    LOCK();
    const Gcr32MultiState *m = low->g32->mw;
    MGCR_CHECK(m && m->k > 0, MGCR_ERR_INVALID, "%s: no batched apply has run on this operator", who);
    G32Dev h[MV_MAX_K];
    MGCR_HIP(hipMemcpyAsync(h, m->st, sizeof(G32Dev) * m->k, hipMemcpyDeviceToHost, ctx().stream));
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    for (int j = 0; j < m->k; j++) {
        if (n_iter) n_iter[j] = h[j].n_iter;
        if (rel_res) rel_res[j] = h[j].rel;
    }
    return MGCR_OK;
}

int mgcr_gcr32_solve_multi(mgcr_op_t A, mgcr_op_t low, double tol, int32_t max_outer, int32_t use_x0, mgcr_mvec_t B, mgcr_mvec_t X, double *hist,
                           int32_t hist_cap, int32_t *n_outer, int32_t *converged) {
    const char *who = "mgcr_gcr32_solve_multi";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(A && B && X, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_TRY(g32m_check_low(low, who));
    MGCR_CHECK(A->kind != OP_DIRAC_MULTI && A->kind != OP_DIRAC_EO_MULTI, MGCR_ERR_UNSUPPORTED,
               "%s: one hopping parameter per column against the one k of the low-precision GCR would not contract", who);
    MGCR_CHECK(max_outer >= 0 && tol >= 0., MGCR_ERR_INVALID, "%s: max_outer and tol must not be negative", who);
    MGCR_CHECK(B->n == X->n && B->k == X->k, MGCR_ERR_INVALID, "%s: B is %lld x %d, X is %lld x %d", who, (long long)B->n, (int)B->k, (long long)X->n,
               (int)X->k);
    MGCR_CHECK(hist_cap >= 0 && (hist || hist_cap == 0), MGCR_ERR_INVALID, "%s: hist_cap without hist", who);
    MGCR_CHECK(B != X && (B->d != X->d || !B->d), MGCR_ERR_INVALID, "%s: B and X must be different blocks", who);
    LOCK();
    Gcr32State *g = low->g32;
    const int k = B->k;
    const int64_t n = B->n;
    mgcr_mvec_s R, E, AX;   // the operator's work blocks, seen as blocks
    {
        mgcr_mvec_s probe;   // the checks of mgcr_op_apply_multi on A, before anything is allocated or changed
        probe.n = (A->nrow ? A->nrow : A->dim);
        probe.k = k;
        MGCR_TRY(op_apply_multi_checks(A, X, &probe, who));
    }
    MGCR_CHECK(A->dim == g->n && (A->nrow ? A->nrow : A->dim) == g->n, MGCR_ERR_INVALID, "%s: the low-precision GCR has %lld rows, the operator of the solve %lld", who,
               (long long)g->n, (long long)A->dim);
    MGCR_TRY(g32m_work(g, k));
    R.n = E.n = AX.n = n;
    R.k = E.k = AX.k = k;
    R.d = g->mw->R; E.d = g->mw->E; AX.d = g->mw->AX;
    double b2[MV_MAX_K], r2[MV_MAX_K], now[MV_MAX_K];
    MGCR_TRY(mgcr_mvec_norm2(B, b2));
    if (use_x0) {
        MGCR_TRY(mgcr_op_apply_multi(A, X, &AX));
        MGCR_TRY(k_add_scaled(R.d, B->d, make_double2(-1., 0.), AX.d, n * k));
    } else {
        MGCR_TRY(k_zero(X->d, n * k));
        MGCR_TRY(mv_copy(R.d, B->d, n, k));
    }
    MGCR_TRY(mgcr_mvec_norm2(&R, r2));
    const double tol2 = tol * tol;
    auto rel = [&](int j) { return b2[j] > 0. ? std::sqrt(r2[j] / b2[j]) : 0.; };
    for (int j = 0; j < k; j++) {
        if (n_outer) n_outer[j] = 0;
        if (hist && hist_cap > 0) hist[(size_t)j * hist_cap] = rel(j);
    }
    for (int t = 1; t <= max_outer; t++) {
        unsigned active = 0;
        for (int j = 0; j < k; j++)
            if (r2[j] > tol2 * b2[j]) active |= 1u << j;   // (b_j = 0: never)
        if (!active) break;
        MGCR_TRY(gcr32_apply_multi(g, R.d, E.d, k, active));
        hipLaunchKernelGGL(g32m_correct_kernel, dim3((unsigned)red_grid(n)), dim3(RED_THREADS), 0, ctx().stream, X->d, (const cplx *)E.d, n, k, active);
        MGCR_HIP(hipGetLastError());
        MGCR_TRY(mgcr_op_apply_multi(A, X, &AX));
        MGCR_TRY(k_add_scaled(R.d, B->d, make_double2(-1., 0.), AX.d, n * k));
        MGCR_TRY(mgcr_mvec_norm2(&R, now));   // the step's one synchronisation
        for (int j = 0; j < k; j++) {
            if (!((active >> j) & 1u)) continue;
            r2[j] = now[j];
            if (n_outer) n_outer[j] = t;
            if (hist && t < hist_cap) hist[(size_t)j * hist_cap + t] = rel(j);
        }
    }
    for (int j = 0; j < k; j++)
        if (converged) converged[j] = !(r2[j] > tol2 * b2[j]) ? 1 : 0;
    return MGCR_OK;
}

}  // extern "C"
