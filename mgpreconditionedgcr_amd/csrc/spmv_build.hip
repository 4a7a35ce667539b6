// Sparse operators on the device, the set-up half: raw CSR (int64, as the reference stores it) -> CsrDev (ELL slab + CSR tail,
// row-pattern dictionary, stencil view, banded window), on the device, and block-CSR -> BcsrDev.  The apply half is spmv.hip;
// the decisions that are pure arithmetic are spmv_layout.h.
#include <algorithm>

#include "internal.h"
#include "spmv_dev.h"
#include "spmv_layout.h"

namespace mgcr {

// one thread per (row, lane): copies the row's first W entries into the slab, pads the rest with
// (last valid column, 0) so that padding never touches an x entry the row does not already read
__global__ void ell_fill_kernel(int64_t nrow, int64_t ncol, const int64_t *__restrict__ rowptr,
                                const int64_t *__restrict__ col, const cplx *__restrict__ val, int32_t W, int32_t L,
                                int32_t nchunk, int64_t npad, cplx *__restrict__ ell_val, int32_t *__restrict__ ell_col) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t row = t / L;
    int32_t l = (int32_t)(t % L);
    if (row >= npad) return;
    int64_t beg = 0, len = 0;
    if (row < nrow) {
        beg = rowptr[row];
        len = rowptr[row + 1] - beg;
    }
    int64_t take = len < W ? len : W;
    int32_t padcol = 0;
    if (take > 0) padcol = (int32_t)col[beg + take - 1];
    else if (row < ncol) padcol = (int32_t)row;
    for (int32_t c = 0; c < nchunk; c++) {
        int32_t w = c * L + l;
        int64_t dst = ((int64_t)c * npad + row) * L + l;
        if (w < take) {
            ell_val[dst] = val[beg + w];
            ell_col[dst] = (int32_t)col[beg + w];
        } else {
            ell_val[dst] = make_double2(0., 0.);
            ell_col[dst] = padcol;
        }
    }
}

__global__ void tail_fill_kernel(int64_t n_tail_rows, const int32_t *__restrict__ tail_rows,
                                 const int32_t *__restrict__ tail_ptr, const int64_t *__restrict__ rowptr,
                                 const int64_t *__restrict__ col, const cplx *__restrict__ val, int32_t W,
                                 int32_t *__restrict__ tail_col, cplx *__restrict__ tail_val) {
    int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (wave >= n_tail_rows) return;
    int64_t row = tail_rows[wave];
    int64_t src = rowptr[row] + W;
    int32_t dst = tail_ptr[wave], cnt = tail_ptr[wave + 1] - dst;
    for (int32_t i = lane; i < cnt; i += 64) {
        tail_col[dst + i] = (int32_t)col[src + i];
        tail_val[dst + i] = val[src + i];
    }
}

// does any value have a non-zero imaginary part?
__global__ void imag_check_kernel(int64_t nnz, const cplx *__restrict__ val, int *__restrict__ has_imag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nnz && val[i].y != 0.) *has_imag = 1;
}
__global__ void slab_real_kernel(int64_t n, const cplx *__restrict__ in, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i].x;
}

// column range check of the uploaded CSR (bad indices would fault inside the SpMV gather)
__global__ void col_check_kernel(int64_t nnz, const int64_t *__restrict__ col, int64_t ncol, int *__restrict__ bad) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nnz && (col[i] < 0 || col[i] >= ncol)) *bad = 1;
}

// Ownership during a build: every device buffer belongs to a DevBuf (internal.h) or to the structure under construction, which a
// BuildGuard frees unless the build hands it over.  So any early return gives back what was allocated.
template <typename D, void (*FREE)(D *)>
struct BuildGuard {
    D d;
    bool mine = true;
    BuildGuard() = default;
    BuildGuard(const BuildGuard &) = delete;
    ~BuildGuard() { if (mine) FREE(&d); }
    void release(D *out) { *out = d; mine = false; }
};

template <typename T>
static int dev_upload(T **d, const T *h, size_t count) {
    *d = nullptr;
    if (count == 0) return MGCR_OK;
    hipError_t e = hipMalloc((void **)d, sizeof(T) * count);
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", sizeof(T) * count, hipGetErrorString(e));
        return MGCR_ERR_ALLOC;
    }
    if (h) MGCR_HIP(hipMemcpyAsync(*d, h, sizeof(T) * count, hipMemcpyHostToDevice, ctx().stream));
    return MGCR_OK;
}

void csr_free(CsrDev *c) {
    hipFree(c->ell_val); hipFree(c->ell_val_re); hipFree(c->ell_col);
    hipFree(c->pat_id); hipFree(c->pat_off); hipFree(c->pat_re); hipFree(c->pat_im); hipFree(c->sten_planes);
    hipFree(c->tail_rows); hipFree(c->tail_ptr); hipFree(c->tail_col); hipFree(c->tail_val);
    hipFree(c->tail_chunk); hipFree(c->tail_long); hipFree(c->win_tile_tail); hipFree(c->win_row_tail);
    *c = CsrDev();
}
void bcsr_free(BcsrDev *b) {
    hipFree(b->browptr); hipFree(b->bcol); hipFree(b->blocks); hipFree(b->order);
    *b = BcsrDev();
}

// ------------------------------------------------------------------------------------------------
// Row-pattern dictionary.  Operators that come from a lattice or a grid repeat a handful of row
// patterns: the tuple (column - row, value) per stored entry is the same for every interior row and
// for every row of a given boundary class (7-point Poisson: 27 patterns for any grid size; Galerkin
// coarse operators of it likewise).  Such a matrix is stored as one 2-byte pattern id per row plus the
// pattern table, which the SpMV reads through L1/L2 — the 12-20 B per stored entry the ELL slab costs
// shrink to 2 B per ROW.  When the values differ from row to row but the sparsity pattern repeats
// (lattice-QCD hopping terms), only the column indices go into the table and the values stay in the slab.
// Entries are multiplied and added in the same order as the ELL kernels do, so y has the same bits.
// The dictionary is found on the device: a hash set of 64-bit row hashes (open addressing, atomicCAS),
// then every row is compared entry by entry with its pattern's first row, so a hash collision can only
// cost the compression (fallback to the plain slab), never correctness.
// ------------------------------------------------------------------------------------------------
constexpr int PAT_TABLE_BITS = 14;  // 16384 slots
constexpr int PAT_MAX = 4096;       // patterns: table stays L2-resident (<= 4096 * W * 20 B)
constexpr int64_t PAT_MIN_ROWS = 1 << 15;

__device__ __forceinline__ uint64_t pat_mix(uint64_t h, uint64_t v) {
    h = (h ^ v) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 29);
}

template <bool VALS>
__device__ __forceinline__ uint64_t pat_row_hash(int64_t i, int64_t npad, int32_t W, const int32_t *__restrict__ col,
                                                 const cplx *__restrict__ val) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int32_t w = 0; w < W; w++) {
        int64_t idx = (int64_t)w * npad + i;
        h = pat_mix(h, (uint64_t)(uint32_t)(col[idx] - (int32_t)i));
        if (VALS) {
            h = pat_mix(h, (uint64_t)__double_as_longlong(val[idx].x));
            h = pat_mix(h, (uint64_t)__double_as_longlong(val[idx].y));
        }
    }
    return h | 1ull;  // 0 marks an empty slot
}

__device__ __forceinline__ int pat_find(uint64_t h, const unsigned long long *keys) {
    const int mask = (1 << PAT_TABLE_BITS) - 1;
    int s = (int)(h >> 20) & mask;
    for (int probe = 0; probe <= mask; probe++) {
        if (keys[s] == h) return s;
        s = (s + 1) & mask;
    }
    return -1;
}

template <bool VALS>
__global__ void pat_insert_kernel(int64_t nrow, int64_t npad, int32_t W, const int32_t *__restrict__ col,
                                  const cplx *__restrict__ val, unsigned long long *keys, int *rep, int *count,
                                  volatile int *overflow) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrow || *overflow) return;
    const uint64_t h = pat_row_hash<VALS>(i, npad, W, col, val);
    const int mask = (1 << PAT_TABLE_BITS) - 1;
    int s = (int)(h >> 20) & mask;
    for (int probe = 0; probe <= mask; probe++) {
        unsigned long long k = *(volatile unsigned long long *)(keys + s);
        if (k == 0ull) {
            k = atomicCAS(keys + s, 0ull, (unsigned long long)h);
            if (k == 0ull) {
                if (atomicAdd(count, 1) + 1 > PAT_MAX) *overflow = 1;
                k = h;
            }
        }
        if (k == h) {
            if ((int)i < *(volatile int *)(rep + s)) atomicMin(rep + s, (int)i);
            return;
        }
        if (*overflow) return;
        s = (s + 1) & mask;
    }
    *overflow = 1;
}

template <bool VALS>
__global__ void pat_assign_kernel(int64_t nrow, int64_t npad, int32_t W, const int32_t *__restrict__ col,
                                  const cplx *__restrict__ val, const unsigned long long *__restrict__ keys,
                                  const int *__restrict__ rep, const int *__restrict__ slot_id, uint16_t *__restrict__ pid,
                                  int *__restrict__ mismatch) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    if (i >= nrow) { pid[i] = 0; return; }
    const uint64_t h = pat_row_hash<VALS>(i, npad, W, col, val);
    int s = pat_find(h, keys);
    if (s < 0) { *mismatch = 1; pid[i] = 0; return; }
    const int64_t r = rep[s];
    bool same = true;
    for (int32_t w = 0; w < W; w++) {
        int64_t a = (int64_t)w * npad + i, b = (int64_t)w * npad + r;
        same = same && (col[a] - (int32_t)i) == (col[b] - (int32_t)r);
        if (VALS)
            same = same && __double_as_longlong(val[a].x) == __double_as_longlong(val[b].x) &&
                   __double_as_longlong(val[a].y) == __double_as_longlong(val[b].y);
    }
    if (!same) *mismatch = 1;
    pid[i] = (uint16_t)slot_id[s];
}

__global__ void pat_fill_kernel(int32_t npat, int32_t W, int64_t npad, const int *__restrict__ rep_row,
                                const int32_t *__restrict__ col, const cplx *__restrict__ val, int32_t *__restrict__ off,
                                double *__restrict__ re, double *__restrict__ im) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npat * W) return;
    int id = t / W, w = t - id * W;
    int64_t r = rep_row[id];
    int64_t idx = (int64_t)w * npad + r;
    off[t] = col[idx] - (int32_t)r;
    if (re) { re[t] = val[idx].x; im[t] = val[idx].y; }
}

static EnvSwitch g_patterns("MGCR_PATTERNS"), g_stencil("MGCR_STENCIL"), g_ell_window("MGCR_ELL_WINDOW"), g_real_storage("MGCR_REAL_STORAGE");
bool set_patterns_enabled(bool on) { return g_patterns.set(on); }
bool set_stencil_enabled(bool on) { return g_stencil.set(on); }
bool stencil_enabled() { return g_stencil.on(); }

// tries to build the dictionary for the (L = 1) slab of A; leaves A.pat_mode = 0 when it does not pay
template <bool VALS>
static int pat_try(CsrDev &A, bool *ok) {
    Context &c = ctx();
    *ok = false;
    const int T = 1 << PAT_TABLE_BITS;
    DevBuf<unsigned long long> d_keys;
    DevBuf<int> d_rep, d_small, d_slot_id, d_rep_row;
    std::vector<unsigned long long> keys((size_t)T);
    std::vector<int> rep((size_t)T), slot_id((size_t)T, 0), small(3, 0);
    int rc = MGCR_OK;
    MGCR_HIP(d_keys.malloc((size_t)T));
    if (!d_rep.alloc((size_t)T) || !d_small.alloc(3) || !d_slot_id.alloc((size_t)T)) return MGCR_OK;  // no memory for the attempt: keep the plain slab
    hipMemsetAsync(d_keys.p, 0, sizeof(unsigned long long) * T, c.stream);
    hipMemsetAsync(d_rep.p, 0x7f, sizeof(int) * T, c.stream);
    hipMemsetAsync(d_small.p, 0, sizeof(int) * 3, c.stream);
    const unsigned grid = (unsigned)((A.nrow + 255) / 256), gridp = (unsigned)((A.npad + 255) / 256);
    hipLaunchKernelGGL((pat_insert_kernel<VALS>), dim3(grid), dim3(256), 0, c.stream, A.nrow, A.npad, A.W, (const int32_t *)A.ell_col,
                       (const cplx *)A.ell_val, d_keys.p, d_rep.p, d_small.p, d_small.p + 1);
    hipMemcpyAsync(small.data(), d_small.p, sizeof(int) * 3, hipMemcpyDeviceToHost, c.stream);
    MGCR_HIP(hipStreamSynchronize(c.stream));
    const int npat = small[0];
    // worth it only when the table is far smaller than the matrix
    if (small[1] || npat < 1 || npat > PAT_MAX || (int64_t)npat * 64 > A.nrow) return MGCR_OK;
    MGCR_HIP(hipMemcpy(keys.data(), d_keys.p, sizeof(unsigned long long) * T, hipMemcpyDeviceToHost));
    MGCR_HIP(hipMemcpy(rep.data(), d_rep.p, sizeof(int) * T, hipMemcpyDeviceToHost));
    // ids in the order of each pattern's first row: deterministic whatever order the inserts raced in
    std::vector<std::pair<int, int>> order;  // (first row, slot)
    for (int s = 0; s < T; s++)
        if (keys[(size_t)s]) order.emplace_back(rep[(size_t)s], s);
    std::sort(order.begin(), order.end());
    if ((int)order.size() != npat) return MGCR_OK;
    std::vector<int> rep_row((size_t)npat);
    for (int id = 0; id < npat; id++) { slot_id[(size_t)order[(size_t)id].second] = id; rep_row[(size_t)id] = order[(size_t)id].first; }
    if (!d_rep_row.alloc((size_t)npat)) return MGCR_OK;
    MGCR_HIP(hipMemcpy(d_slot_id.p, slot_id.data(), sizeof(int) * T, hipMemcpyHostToDevice));
    MGCR_HIP(hipMemcpy(d_rep_row.p, rep_row.data(), sizeof(int) * npat, hipMemcpyHostToDevice));
    DevBuf<uint16_t> pid;
    DevBuf<int32_t> off;
    DevBuf<double> re, im;
    const bool alloc_ok = pid.alloc((size_t)A.npad) && off.alloc((size_t)npat * A.W) &&
                          (!VALS || (re.alloc((size_t)npat * A.W) && im.alloc((size_t)npat * A.W)));
    if (alloc_ok) {
        hipLaunchKernelGGL((pat_assign_kernel<VALS>), dim3(gridp), dim3(256), 0, c.stream, A.nrow, A.npad, A.W,
                           (const int32_t *)A.ell_col, (const cplx *)A.ell_val, (const unsigned long long *)d_keys.p, (const int *)d_rep.p,
                           (const int *)d_slot_id.p, pid.p, d_small.p + 2);
        hipLaunchKernelGGL(pat_fill_kernel, dim3((unsigned)((npat * A.W + 255) / 256)), dim3(256), 0, c.stream, npat, A.W, A.npad,
                           (const int *)d_rep_row.p, (const int32_t *)A.ell_col, (const cplx *)A.ell_val, off.p, re.p, im.p);
        hipMemcpyAsync(small.data(), d_small.p, sizeof(int) * 3, hipMemcpyDeviceToHost, c.stream);
        if (hipStreamSynchronize(c.stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = MGCR_ERR_HIP;
    }
    if (!alloc_ok || rc != MGCR_OK || small[2]) {  // small[2]: two different rows shared a hash
        if (rc != MGCR_OK) set_error("pattern dictionary kernels failed");
        return rc;
    }
    {   // how far the gathers of a row reach (decides the row -> workgroup map of the GCR step kernels, gcr_dev.h)
        std::vector<int32_t> h_off((size_t)npat * A.W);
        if (hipMemcpy(h_off.data(), off.p, sizeof(int32_t) * h_off.size(), hipMemcpyDeviceToHost) == hipSuccess)
            for (int32_t o : h_off) A.reach = std::max<int64_t>(A.reach, o < 0 ? -(int64_t)o : (int64_t)o);
    }
    A.pat_mode = VALS ? 1 : 2;
    A.npat = npat;
    A.pat_id = pid.release(); A.pat_off = off.release(); A.pat_re = re.release(); A.pat_im = im.release();
    *ok = true;
    return MGCR_OK;
}

// ------------------------------------------------------------------------------------------------
// Stencil view of a mode-1 dictionary (CsrDev::sten_*; kernels: spmv.hip sten_spmv, MODE 3 of the fused GCR step
// kernels).  The dictionary kernels are bound by a dependent chain per row — id -> table -> gathers, two memory round
// trips — not by bandwidth.  When all patterns are sub-stencils of one small stencil (their column offsets are
// subsequences of one ascending list of at most STEN_MAX offsets) and a slot's value is the same in every pattern that
// has it — the 7-point Poisson matrix, its Galerkin coarse operators, any constant-coefficient stencil with
// truncated boundaries — a row needs only to know WHICH slots it has: one bit per row and slot, stored as one 64-bit
// word per wave of 64 rows and slot and read through the scalar cache.  The x loads then depend on the row number
// alone (coalesced, wave-uniform offsets) and are in flight while the presence words arrive.  Measured on MI355X
// (tools/spmv_lab.hip, Poisson): 13.1 against 16.8 us at 128^3 back to back, 134 against 168 us at 256^3.
// Entries whose stored value is exactly 0 (the slab's padding) are treated as absent: they only ever add +-0.
// ------------------------------------------------------------------------------------------------
// (each wave walks several waves' worth of rows and keeps the per-slot row counts in lane 0's registers: one atomic per slot and
// WAVE OF THE GRID at the end.  One atomic per slot and 64 rows — 2.3 M of them on 16 addresses at 256^3 — took 25 ms.)
__global__ void __launch_bounds__(256) sten_planes_kernel(int64_t nrow, int64_t nwaves, int32_t ns, int32_t stride,
                                                          const uint16_t *__restrict__ pid, const uint16_t *__restrict__ pmask,
                                                          uint64_t *__restrict__ planes, unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t gw = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, tw = (int64_t)gridDim.x * 4;
    unsigned long long cnt[16];
#pragma unroll
    for (int c = 0; c < 16; c++) cnt[c] = 0ull;
    for (int64_t wave = gw; wave < nwaves; wave += tw) {
        const int64_t row = wave * 64 + lane;
        const uint32_t m = row < nrow ? pmask[pid[row]] : 0u;
#pragma unroll
        for (int32_t c = 0; c < 16; c++) {
            if (c < stride) {
                const unsigned long long b = __ballot(c < ns && (m >> c & 1u));
                if (lane == 0) planes[wave * stride + c] = b;
                cnt[c] += (unsigned long long)__popcll(b);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 16; c++)
            if (cnt[c]) atomicAdd(counts + c, cnt[c]);
    }
}

// presence words of A's rows for the slot numbering `pm` (pattern -> mask), `stride` words per wave; counts[k] = rows that have slot k
static bool sten_presence(const CsrDev &A, const std::vector<uint16_t> &pm, int nslots, int32_t stride, uint16_t *d_pmask,
                          unsigned long long *d_counts, uint64_t *planes, std::vector<unsigned long long> &counts) {
    Context &c = ctx();
    const int64_t nwaves = A.npad / 64;
    counts.assign(16, 0);
    bool g = hipMemcpyAsync(d_pmask, pm.data(), sizeof(uint16_t) * (size_t)A.npat, hipMemcpyHostToDevice, c.stream) == hipSuccess &&
             hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * 16, c.stream) == hipSuccess &&
             hipMemsetAsync(planes + (size_t)nwaves * stride, 0, sizeof(uint64_t) * stride, c.stream) == hipSuccess;
    if (g && nwaves) {
        const int64_t pg = (nwaves + 3) / 4;   // 4 waves per workgroup; at most 2048 workgroups, each wave then walks several
        hipLaunchKernelGGL(sten_planes_kernel, dim3((unsigned)(pg < 2048 ? pg : 2048)), dim3(256), 0, c.stream, A.nrow, nwaves, nslots,
                           stride, (const uint16_t *)A.pat_id, (const uint16_t *)d_pmask, planes, d_counts);
        g = hipGetLastError() == hipSuccess;
    }
    return g && hipMemcpyAsync(counts.data(), d_counts, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, c.stream) == hipSuccess &&
           hipStreamSynchronize(c.stream) == hipSuccess;
}

// builds the stencil view of A (pat_mode 1) when the dictionary has that shape; leaves A.sten_ns = 0 otherwise:
// download the table, stage 1, presence pass (which rows have which slot), stage 2, presence pass in kernel layout, store
static int sten_try(CsrDev &A) {
    A.sten_ns = 0;
    if (A.pat_mode != 1 || A.npat < 1 || !g_stencil.on()) return MGCR_OK;
    const size_t ne = (size_t)A.npat * A.W;
    std::vector<int32_t> off(ne);
    std::vector<double> re(ne), im(ne);
    MGCR_HIP(hipMemcpy(off.data(), A.pat_off, sizeof(int32_t) * ne, hipMemcpyDeviceToHost));
    MGCR_HIP(hipMemcpy(re.data(), A.pat_re, sizeof(double) * ne, hipMemcpyDeviceToHost));
    MGCR_HIP(hipMemcpy(im.data(), A.pat_im, sizeof(double) * ne, hipMemcpyDeviceToHost));
    const StenSlots s1 = sten_stage1(off, re, im, A.npat, A.W, STEN_MAX);
    if (!s1.view) return MGCR_OK;
    DevBuf<uint16_t> d_pmask;
    DevBuf<unsigned long long> d_counts;
    DevBuf<uint64_t> planes;
    std::vector<unsigned long long> counts;
    auto no_memory = [] { (void)hipGetLastError(); return MGCR_OK; };   // no memory for the view: the dictionary kernels stay
    if (!d_pmask.alloc((size_t)A.npat) || !d_counts.alloc(16) || !planes.alloc((size_t)(A.npad / 64 + 1) * 16) ||
        !sten_presence(A, s1.pbits, (int)s1.S.size(), 16, d_pmask.p, d_counts.p, planes.p, counts))
        return no_memory();
    const bool force = getenv("MGCR_TEST_FORCE_RARE") && atoi(getenv("MGCR_TEST_FORCE_RARE")) != 0;   // read at every build
    const StenLayout lay = sten_stage2(s1, counts, A.nrow, force, StenLimits{STEN_COMMON, STEN_TILE / 2, RED_THREADS / 2});
    if (!lay.view) return MGCR_OK;
    if (!sten_presence(A, lay.pmask, lay.kernel_ns, lay.stride, d_pmask.p, d_counts.p, planes.p, counts)) return no_memory();
    A.sten_ns = (int32_t)s1.S.size(); A.sten_kernel_ns = lay.kernel_ns; A.sten_stride = lay.stride;
    A.sten_planes = planes.release(); A.sten_rare = lay.rare; A.sten_pre = lay.pre;
    for (int k = 0; k < 16; k++) { A.sten_off[k] = lay.off[k]; A.sten_re[k] = lay.re[k]; A.sten_im[k] = lay.im[k]; }
    A.sten_near = lay.near; A.sten_halo = lay.halo; A.sten_near_f = lay.near_f; A.sten_halo_f = lay.halo_f;
    if (lay.reach >= 0) A.reach = lay.reach;
    return MGCR_OK;
}

// Banded irregular matrices (FEM / graph matrices in a bandwidth-reducing order): the gathers of x, one L2 request of 128 B per
// 16-byte entry, are what bounds the slab kernel (profiles/r03_gather_lab.txt); with >= 90 % of the columns within H rows of the
// row the window kernel reads x[tile - H, tile + 1024 + H) once, coalesced, into LDS and gathers from there.
static int ell_window_try(CsrDev &A) {
    A.win_h = 0;
    if (!g_ell_window.on()) return MGCR_OK;
    DevBuf<unsigned long long> d_cnt;
    unsigned long long h_cnt[2] = {0, 0};
    MGCR_HIP(d_cnt.malloc(2));
    MGCR_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), ctx().stream));
    MGCR_TRY(ell_band_count(A, d_cnt.p));
    MGCR_HIP(hipMemcpyAsync(h_cnt, d_cnt.p, sizeof(h_cnt), hipMemcpyDeviceToHost, ctx().stream));
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    const double slots = (double)A.nrow * A.W;
    if ((double)h_cnt[0] >= 0.9 * slots) A.win_h = 1024;
    else if ((double)h_cnt[1] >= 0.9 * slots) A.win_h = 4096;
    return MGCR_OK;
}

// ---- the steps of csr_build_from_device; A is the CsrDev under construction (its guard frees it on any failure) ----
static int slab_fill(CsrDev &A, size_t slab, const int64_t *d_rowptr, const int64_t *d_col, const cplx *d_val) {
    hipError_t e1 = hipMalloc((void **)&A.ell_val, sizeof(cplx) * slab);
    hipError_t e2 = hipMalloc((void **)&A.ell_col, sizeof(int32_t) * slab);
    MGCR_CHECK(e1 == hipSuccess && e2 == hipSuccess, MGCR_ERR_ALLOC, "hipMalloc of the ELL slab (%zu entries) failed", slab);
    int64_t threads = A.npad * A.L;
    hipLaunchKernelGGL(ell_fill_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx().stream, A.nrow, A.ncol,
                       d_rowptr, d_col, d_val, A.W, A.L, A.nchunk, A.npad, A.ell_val, A.ell_col);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

// (the caller keeps the four lists alive until the stream has run the uploads)
static int tail_fill(CsrDev &A, const std::vector<int32_t> &trows, const std::vector<int32_t> &tptr, const std::vector<TailChunk> &chunks,
                     const std::vector<int32_t> &long_rows, const int64_t *d_rowptr, const int64_t *d_col, const cplx *d_val) {
    static_assert(sizeof(TailChunk) == sizeof(int4), "TailChunk is uploaded as CsrDev::tail_chunk");
    A.n_tail_chunks = (int32_t)chunks.size();
    A.n_tail_long = (int32_t)long_rows.size();
    if (A.n_tail_chunks) MGCR_TRY(dev_upload(&A.tail_chunk, (const int4 *)chunks.data(), chunks.size()));
    if (A.n_tail_long) MGCR_TRY(dev_upload(&A.tail_long, long_rows.data(), long_rows.size()));
    MGCR_TRY(dev_upload(&A.tail_rows, trows.data(), trows.size()));
    MGCR_TRY(dev_upload(&A.tail_ptr, tptr.data(), tptr.size()));
    MGCR_TRY(dev_upload<int32_t>(&A.tail_col, nullptr, (size_t)A.tail_nnz));
    MGCR_TRY(dev_upload<cplx>(&A.tail_val, nullptr, (size_t)A.tail_nnz));
    int64_t threads = A.n_tail_rows * 64;
    hipLaunchKernelGGL(tail_fill_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx().stream,
                       A.n_tail_rows, A.tail_rows, A.tail_ptr, d_rowptr, d_col, d_val, A.W, A.tail_col, A.tail_val);
    MGCR_HIP(hipGetLastError());
    return MGCR_OK;
}

// dictionary with values (then the slab goes, and the stencil view is tried: *table_only), else dictionary of the columns
static int dictionary_try(CsrDev &A, int has_imag, bool *table_only) {
    MGCR_TRY(pat_try<true>(A, table_only));
    if (*table_only) {  // the table holds everything: no slab
        A.pat_real = !has_imag;
        hipFree(A.ell_val); hipFree(A.ell_col);
        A.ell_val = nullptr; A.ell_col = nullptr;
        return sten_try(A);
    }
    bool ok = false;
    MGCR_TRY(pat_try<false>(A, &ok));
    if (ok) { hipFree(A.ell_col); A.ell_col = nullptr; }
    return MGCR_OK;
}

// device-resident CSR (int64 indices) -> ELL + tail; h_rowptr is the host copy of the row pointers
int csr_build_from_device(int64_t nrow, int64_t ncol, const int64_t *h_rowptr, const int64_t *d_rowptr, const int64_t *d_col,
                          const cplx *d_val, CsrDev *out) {
    Context &c = ctx();
    BuildGuard<CsrDev, csr_free> build;   // A: the CsrDev under construction
    CsrDev &A = build.d;
    A.nrow = nrow; A.ncol = ncol; A.nnz = h_rowptr[nrow];
    int64_t maxlen64 = 0;
    for (int64_t r = 0; r < nrow; r++) maxlen64 = std::max(maxlen64, h_rowptr[r + 1] - h_rowptr[r]);
    MGCR_CHECK(maxlen64 < ((int64_t)1 << 30), MGCR_ERR_UNSUPPORTED, "row with %lld entries", (long long)maxlen64);
    int32_t maxlen = (int32_t)maxlen64;
    std::vector<int64_t> hist((size_t)maxlen + 2, 0);
    for (int64_t r = 0; r < nrow; r++) hist[(size_t)(h_rowptr[r + 1] - h_rowptr[r])]++;
    A.W = choose_width(hist, nrow, maxlen);
    A.L = choose_lanes(nrow, A.W);
    A.nchunk = (A.W + A.L - 1) / A.L;
    A.npad = (nrow + 63) / 64 * 64;
    // tail lists
    std::vector<int32_t> trows, tptr(1, 0);
    for (int64_t r = 0; r < nrow; r++) {
        int64_t len = h_rowptr[r + 1] - h_rowptr[r];
        if (len > A.W) {
            trows.push_back((int32_t)r);
            int64_t nxt = (int64_t)tptr.back() + (len - A.W);
            MGCR_CHECK(nxt < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED, "CSR tail exceeds 2^31 entries");
            tptr.push_back((int32_t)nxt);
        }
    }
    A.n_tail_rows = (int64_t)trows.size();
    A.tail_nnz = tptr.back();
    const size_t slab = (size_t)A.nchunk * (size_t)A.npad * (size_t)A.L;
    if (slab) MGCR_TRY(slab_fill(A, slab, d_rowptr, d_col, d_val));
    std::vector<TailChunk> chunks;
    std::vector<int32_t> long_rows;
    if (A.n_tail_rows) {
        deal_tail(tptr, TAIL_CAP, TAIL_THREADS, chunks, long_rows);
        MGCR_TRY(tail_fill(A, trows, tptr, chunks, long_rows, d_rowptr, d_col, d_val));
    }
    MGCR_HIP(hipStreamSynchronize(c.stream));  // the lists' uploads are done
    int has_imag = 1;
    if (slab && A.nnz > 0) {
        DevBuf<int> d_flag;
        MGCR_HIP(d_flag.malloc(1));
        MGCR_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(int), c.stream));
        hipLaunchKernelGGL(imag_check_kernel, dim3((unsigned)((A.nnz + 255) / 256)), dim3(256), 0, c.stream, A.nnz, d_val, d_flag.p);
        MGCR_HIP(hipMemcpyAsync(&has_imag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        MGCR_HIP(hipStreamSynchronize(c.stream));
    }
    if (slab && A.L == 1 && A.W >= 1 && A.W <= 32 && A.nrow >= PAT_MIN_ROWS && g_patterns.on()) {
        bool table_only = false;
        MGCR_TRY(dictionary_try(A, has_imag, &table_only));
        if (table_only) { build.release(out); return MGCR_OK; }
    }
    if (slab && A.L == 1 && A.pat_mode == 0 && A.nrow == A.ncol && A.nrow >= ELL_WIN_ROWS && A.W >= 2) MGCR_TRY(ell_window_try(A));
    if (A.win_h && A.n_tail_rows) {
        std::vector<int32_t> tile_tail, row_tail;
        window_tail_tables(trows, tptr, A.nrow, ELL_WIN_ROWS, TAIL_CAP, tile_tail, row_tail);
        MGCR_TRY(dev_upload(&A.win_tile_tail, tile_tail.data(), tile_tail.size()));
        MGCR_TRY(dev_upload(&A.win_row_tail, row_tail.data(), row_tail.size()));
        MGCR_HIP(hipStreamSynchronize(ctx().stream));
    }
    // Real matrices (every imaginary part exactly 0, e.g. Poisson): keep the slab's values as fp64
    // reals, 12 B instead of 20 B per stored entry.  v*(c+di) with v real is (vc, vd): the same numbers
    // the complex product (vc - 0*d, vd + 0*c) gives for finite x.
    if (slab && A.nnz > 0 && g_real_storage.on() && !has_imag && hipMalloc((void **)&A.ell_val_re, sizeof(double) * slab) == hipSuccess) {
        hipLaunchKernelGGL(slab_real_kernel, dim3((unsigned)((slab + 255) / 256)), dim3(256), 0, c.stream, (int64_t)slab,
                           (const cplx *)A.ell_val, A.ell_val_re);
        MGCR_HIP(hipStreamSynchronize(c.stream));
        hipFree(A.ell_val);
        A.ell_val = nullptr;
    }
    build.release(out);
    return MGCR_OK;
}

int csr_build_device(int64_t nrow, int64_t ncol, const int64_t *h_rowptr, const int64_t *h_col, const double *h_val_ri,
                     CsrDev *out) {
    Context &c = ctx();
    MGCR_CHECK(nrow >= 0 && ncol >= 0 && nrow < ((int64_t)1 << 31) && ncol < ((int64_t)1 << 31), MGCR_ERR_UNSUPPORTED,
               "matrix dimensions must fit int32 per GPU (got %lld x %lld)", (long long)nrow, (long long)ncol);
    MGCR_CHECK(h_rowptr[0] == 0, MGCR_ERR_INVALID, "rowptr[0] must be 0");
    for (int64_t r = 0; r < nrow; r++)
        MGCR_CHECK(h_rowptr[r + 1] >= h_rowptr[r], MGCR_ERR_INVALID, "rowptr is not non-decreasing at row %lld", (long long)r);
    int64_t nnz = h_rowptr[nrow];
    DevBuf<int64_t> d_rowptr, d_col;
    DevBuf<cplx> d_val;
    DevBuf<int> d_bad;
    int rc = dev_upload(&d_rowptr.p, h_rowptr, (size_t)nrow + 1);
    if (rc == MGCR_OK) rc = dev_upload(&d_col.p, h_col, (size_t)nnz);
    if (rc == MGCR_OK) rc = dev_upload(&d_val.p, (const cplx *)h_val_ri, (size_t)nnz);
    int bad = 0;
    if (rc == MGCR_OK && nnz > 0) {
        rc = dev_upload(&d_bad.p, &bad, 1);
        if (rc == MGCR_OK) {
            hipLaunchKernelGGL(col_check_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, c.stream, nnz, d_col.p, ncol, d_bad.p);
            hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, c.stream);
            hipStreamSynchronize(c.stream);
            if (bad) { set_error("mgcr_csr_create: a column index is outside [0, ncol)"); rc = MGCR_ERR_INVALID; }
        }
    }
    if (rc == MGCR_OK) rc = csr_build_from_device(nrow, ncol, h_rowptr, d_rowptr.p, d_col.p, d_val.p, out);
    hipStreamSynchronize(c.stream);   // (before the four uploads are freed)
    return rc;
}

int bcsr_build_device(int32_t nbrow, int32_t nbcol, int32_t bs, const int32_t *h_browptr, const int32_t *h_bcol,
                      const double *h_blocks, BcsrDev *out) {
    MGCR_CHECK(nbrow >= 0 && nbcol >= 0 && bs >= 1 && bs <= 128, MGCR_ERR_UNSUPPORTED,
               "block-CSR: block size must be in [1,128] (got %d)", bs);
    MGCR_CHECK(h_browptr[0] == 0, MGCR_ERR_INVALID, "browptr[0] must be 0");
    for (int32_t r = 0; r < nbrow; r++) MGCR_CHECK(h_browptr[r + 1] >= h_browptr[r], MGCR_ERR_INVALID, "browptr not monotone");
    int32_t nb = h_browptr[nbrow];
    for (int32_t i = 0; i < nb; i++) MGCR_CHECK(h_bcol[i] >= 0 && h_bcol[i] < nbcol, MGCR_ERR_INVALID, "block column out of range");
    BuildGuard<BcsrDev, bcsr_free> build;
    BcsrDev &B = build.d;
    B.nbrow = nbrow; B.nbcol = nbcol; B.bs = bs; B.nblocks = nb;
    MGCR_TRY(dev_upload(&B.browptr, h_browptr, (size_t)nbrow + 1));
    MGCR_TRY(dev_upload(&B.bcol, h_bcol, (size_t)nb));
    MGCR_TRY(dev_upload(&B.blocks, (const cplx *)h_blocks, (size_t)nb * bs * bs));
    // One wave per block row, rows of 5 .. 64 blocks: dealt in stored order, the rows that happen to come last decide when the
    // kernel ends (a 64-block row started near the end runs almost alone).  Longest rows first (stable: equal counts keep
    // their order) — each row is still summed by one wave in its own order, so the result does not change by a bit.
    static EnvSwitch lpt("MGCR_BCSR_ORDER");
    if (lpt.on() && nbrow >= 1024) {
        int32_t cmin = INT32_MAX, cmax = 0;
        for (int32_t r = 0; r < nbrow; r++) {
            const int32_t c = h_browptr[r + 1] - h_browptr[r];
            cmin = std::min(cmin, c); cmax = std::max(cmax, c);
        }
        if (cmax > cmin) {
            std::vector<int32_t> order((size_t)nbrow);
            for (int32_t r = 0; r < nbrow; r++) order[(size_t)r] = r;
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
                return h_browptr[a + 1] - h_browptr[a] > h_browptr[b + 1] - h_browptr[b];
            });
            MGCR_TRY(dev_upload(&B.order, order.data(), (size_t)nbrow));
        }
    }
    MGCR_HIP(hipStreamSynchronize(ctx().stream));
    build.release(out);
    return MGCR_OK;
}

}  // namespace mgcr
