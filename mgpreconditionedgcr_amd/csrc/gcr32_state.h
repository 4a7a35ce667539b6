// The state of a low-precision GCR (OP_GCR32), shared by gcr32.hip, which owns the inner solve, and gcr32_eo.hip, whose operator is
// the fp32 even-odd Schur complement: the device-side words of the solve, the fp32 slab of one matrix and the storage of the
// iteration.  Host and device declarations only — the row sum itself is gcr32_row_dev.h.
#pragma once
#include <vector>

#include "gcr32_plan.h"
#include "internal.h"
#include "reduce.h"

namespace mgcr {

typedef float2 c32;
constexpr int G32_TILE = RED_THREADS;   // rows per workgroup of the apply (one thread per row)

struct G32Dev {
    int stop_a;    // steps the solve was cut to by the tolerance (INT_MAX: running); written by the apply kernels only
    int stop_u;    // ... by a zero <Ap, Ap>; written by the update kernels only
    int n_iter;    // steps performed
    double rel;    // fp32 |r| / |f| behind the last step (exit kernel)
    double den[GCR32_MAX_RESTART];   // <Ap_j, Ap_j> of the stored directions
};

struct G32Mat {
    const float *val;       // [W][npad] or [W][npad][2]
    const int32_t *col;     // [W][npad], -1: padding
    int64_t npad;
    int32_t W;
    const int32_t *tile_tail, *tail_rows, *tail_ptr, *tail_col;
    const float *tail_val;
};

struct Gcr32EoState;   // gcr32_eo.hip
struct Gcr32MultiState;   // gcr32_multi.hip

struct Gcr32State {
    int64_t n = 0, nv = 0, nnz = 0, n_tail_rows = 0, stored_bytes = 0;
    int32_t W = 0;
    bool real = false, dirac = false;
    double k_ri[2] = {0., 0.};
    c32 k32 = {0.f, 0.f};
    int restart = 0, max_iter = 0;
    double tol = 0.;
    float *val = nullptr, *tail_val = nullptr;
    int32_t *col = nullptr, *tile_tail = nullptr, *tail_rows = nullptr, *tail_ptr = nullptr, *tail_col = nullptr;
    int64_t npad = 0;
    float *r = nullptr, *ar = nullptr, *x = nullptr, *ps = nullptr, *aps = nullptr;   // c32 vectors of nv elements; ps, aps: restart slots
    double *S2 = nullptr;       // [2][RED_MAX_BLOCKS]: |f|^2, |r|^2
    double *partsA = nullptr;   // [3][RED_MAX_BLOCKS]: <Ap, Ap>, <Ap, r>
    double *partsB = nullptr;   // [2 * GCR32_MAX_RESTART][RED_MAX_BLOCKS]: <Ap_j, Ar>
    G32Dev *st = nullptr;
    Gcr32EoState *eo = nullptr;   // the even-odd form (mgcr_gcr32_create_eo): n = n_e, the matrix fields above are unused (owned)
    Gcr32MultiState *mw = nullptr;   // the k-wide storage of mgcr_gcr32_apply_multi, made by its first call (owned)
};

#define SKIP_ARGS const int *__restrict__ skip, int skip_it
#define SKIP_RETURN() \
    if (skip && skip[0] < skip[1] + skip_it) return

// NV block sums into a partial slab, at most 16 scalars at a time (each scalar's tree is wave_sum's whatever the chunking)
template <int NV, int OFF = 0>
__device__ __forceinline__ void block_sums_to_slab(const double (&acc)[NV], double *lds, double *__restrict__ parts, int blk) {
    constexpr int C = NV - OFF < 16 ? NV - OFF : 16;
    double v[C];
#pragma unroll
    for (int j = 0; j < C; j++) v[j] = acc[OFF + j];
    const double mine = block_sum_owner<C>(v, lds + OFF * 17);
    if ((int)threadIdx.x < C) parts[(size_t)(OFF + threadIdx.x) * RED_MAX_BLOCKS + blk] = mine;
    if constexpr (OFF + C < NV) block_sums_to_slab<NV, OFF + C>(acc, lds, parts, blk);
}

template <typename T>
static int g32_alloc(T **p, size_t count) {
    hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", sizeof(T) * count, hipGetErrorString(e));
        return MGCR_ERR_ALLOC;
    }
    return MGCR_OK;
}
template <typename T>
static int g32_upload(T **p, const std::vector<T> &h) {
    MGCR_TRY(g32_alloc(p, h.size()));
    if (!h.empty()) MGCR_HIP(hipMemcpy(*p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return MGCR_OK;
}

// ---- gcr32.hip's host pieces that gcr32_eo.hip builds on --------------------------------------------------------------------------
int g32_check_param(const mgcr_gcr_param *p, const char *who);
int g32_check_k(const double k_ri[2], c32 *k32, const char *who);
// the storage of the iteration (r, Ar, x, the slots, the partial slabs, the state words, the library's counters) for g->n rows
int g32_alloc_iteration(Gcr32State *g);

// ---- gcr32_eo.hip: the apply of the even-odd form --------------------------------------------------------------------------------
void gcr32_eo_destroy(Gcr32EoState *e);
int gcr32_eo_launch_apply(Gcr32State *g, int nd, int it, SkipRef sk);   // stage 1 + stage 2: Ar = S32 r and the partials of <Ap_j, Ar>
int gcr32_eo_set_k(Gcr32State *g, const double k_ri[2], const char *who);   // refused: nothing changes
// the slot check's questions about a preconditioner in even-odd form and about the operator of the solve
int gcr32_eo_slot_check(const Gcr32EoState *e, const Op *A);

// ---- gcr32_multi.hip: the k-wide lockstep inner solve ------------------------------------------------------------------------------
void gcr32_multi_destroy(Gcr32MultiState *m);

// ---- gcr_multi_flex.hip: the two launches a k-wide apply takes on when an outer batched solve hands it its state (MFlexGate) ----------
int mflex_gate(const MFlexGate &g, int k, G32Dev *st32);
int mflex_exit(const MFlexGate &g, const c32 *x, cplx *y, int64_t nv, int64_t n, int k, const double *S2, int nblkS, G32Dev *st32);

}  // namespace mgcr
