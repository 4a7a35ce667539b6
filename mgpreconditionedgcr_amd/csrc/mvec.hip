// Multi-vector ("block of k Fields") part of the C ABI: storage, host <-> device transposition, column pack / unpack and
// the block BLAS-1 (k dot products / norms in ONE pass, per-column axpy).  Layout and thread mapping: multi_dev.h.
#include "internal.h"
#include "reduce.h"
#include "multi_dev.h"

namespace mgcr {

// dev[i * k + c] = stage[c * n + i] (TO_DEV) or the reverse: the [k][n] <-> [n][k] transposition of an upload / download
template <bool TO_DEV>
__global__ void __launch_bounds__(RED_THREADS) mv_transpose_kernel(cplx *__restrict__ dst, const cplx *__restrict__ src, int64_t n, int k) {
    MV_GRID_STRIDE(e, n * k) {
        const int64_t i = e / k;
        const int c = (int)(e - i * k);
        if (TO_DEV) dst[e] = src[(int64_t)c * n + i];
        else dst[(int64_t)c * n + i] = src[e];
    }
}
// column j of a multi-vector <-> a Field
template <bool SET>
__global__ void __launch_bounds__(RED_THREADS) mv_column_kernel(cplx *__restrict__ mv, cplx *__restrict__ f, int64_t n, int k, int j) {
    MV_GRID_STRIDE(i, n) {
        if (SET) mv[i * k + j] = f[i];
        else f[i] = mv[i * k + j];
    }
}
__global__ void __launch_bounds__(RED_THREADS) mv_copy_kernel(cplx *__restrict__ dst, const cplx *__restrict__ src, int64_t ne) {
    MV_GRID_STRIDE(e, ne) dst[e] = src[e];
}

// partial sums of conj(a_ij) b_ij per column j -> parts[2 j][blk] (re), parts[2 j + 1][blk] (im): dot_partials_kernel (blas1.hip)
// once per column inside one pass over a and b
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) mv_dot_kernel(const cplx *__restrict__ a, const cplx *__restrict__ b, int64_t n, int k,
                                                             double *__restrict__ parts) {
    __shared__ double lds[2 * KC * 17];
    const int c0 = (int)blockIdx.y * KC;
    double v[2 * KC];
#pragma unroll
    for (int s = 0; s < 2 * KC; s++) v[s] = 0.;
    MV_GRID_STRIDE(i, n) {
        cplx av[KC], bv[KC];
        mv_load<KC>(a, i, k, c0, av);
        mv_load<KC>(b, i, k, c0, bv);
#pragma unroll
        for (int c = 0; c < KC; c++) {
            const cplx t = cconj_mul(av[c], bv[c]);
            v[2 * c] += t.x;
            v[2 * c + 1] += t.y;
        }
    }
    const double tot = block_sum_owner<2 * KC>(v, lds);
    const int t = (int)threadIdx.x;
    if (t < 2 * KC && c0 + t / 2 < k) parts[(size_t)(2 * c0 + t) * RED_MAX_BLOCKS + blockIdx.x] = tot;
}

struct MvAlpha {
    cplx a[MV_MAX_K];
};
// y_j += alpha_j x_j, the arithmetic of add_scaled_kernel per column
template <int KC>
__global__ void __launch_bounds__(RED_THREADS) mv_axpy_kernel(MvAlpha al, const cplx *__restrict__ x, cplx *__restrict__ y, int64_t n, int k) {
    const int c0 = (int)blockIdx.y * KC;
    MV_GRID_STRIDE(i, n) {
        cplx xv[KC], yv[KC];
        mv_load<KC>(x, i, k, c0, xv);
        mv_load<KC>(y, i, k, c0, yv);
#pragma unroll
        for (int c = 0; c < KC; c++)
            if (c0 + c < k) y[i * k + c0 + c] = cadd(yv[c], cmul(al.a[c0 + c], xv[c]));
    }
}

#define MV_LAUNCH(kernel, grid, ...)                                                               \
    do {                                                                                           \
        hipLaunchKernelGGL(kernel, grid, dim3(RED_THREADS), 0, ctx().stream, __VA_ARGS__);         \
        MGCR_HIP(hipGetLastError());                                                               \
    } while (0)
// launches kernel<KC> with KC = mv_group(k) over (g, ceil(k / KC)) workgroups
#define MV_LAUNCH_KC(kernel, g, k, ...)                                                            \
    do {                                                                                           \
        const int kc__ = mv_group(k);                                                              \
        const dim3 grid__((unsigned)(g), (unsigned)(((k) + kc__ - 1) / kc__));                     \
        if (kc__ == 1) MV_LAUNCH((kernel<1>), grid__, __VA_ARGS__);                                \
        else if (kc__ == 2) MV_LAUNCH((kernel<2>), grid__, __VA_ARGS__);                           \
        else MV_LAUNCH((kernel<4>), grid__, __VA_ARGS__);                                          \
    } while (0)

int mv_copy(cplx *dst, const cplx *src, int64_t n, int k) {
    if (n == 0 || dst == src) return MGCR_OK;
    MV_LAUNCH(mv_copy_kernel, dim3((unsigned)red_grid(n * k)), dst, src, n * k);
    return MGCR_OK;
}

// k dots (conj on a) to the host: out_ri[2 j], out_ri[2 j + 1]
static double *g_dot_parts = nullptr, *g_dot_res = nullptr;   // released with the context (multi_release)
void mvec_release() {
    hipFree(g_dot_parts);
    hipFree(g_dot_res);
    g_dot_parts = g_dot_res = nullptr;
}
static int mv_dot_to_host(const cplx *a, const cplx *b, int64_t n, int k, double *out_ri) {
    Context &c = ctx();
    double *&parts = g_dot_parts, *&dres = g_dot_res;
    if (!parts) {
        MGCR_HIP(hipMalloc((void **)&parts, sizeof(double) * 2 * MV_MAX_K * RED_MAX_BLOCKS));
        MGCR_HIP(hipMalloc((void **)&dres, sizeof(double) * 2 * MV_MAX_K));
    }
    const int g = red_grid(n);   // the rows are dealt as mgcr_dot deals them
    MV_LAUNCH_KC(mv_dot_kernel, g, k, a, b, n, k, parts);
    MGCR_TRY(k_fold(parts, g, 2 * k, dres));
    MGCR_HIP(hipMemcpyAsync(c.h_mail, dres, 2 * k * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    MGCR_HIP(hipStreamSynchronize(c.stream));
    for (int s = 0; s < 2 * k; s++) out_ri[s] = c.h_mail[s];
    return MGCR_OK;
}

}  // namespace mgcr

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_mvec_create(int64_t n, int32_t k, mgcr_mvec_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && n >= 0, MGCR_ERR_INVALID, "mgcr_mvec_create: bad arguments");
    MGCR_CHECK(k >= 1 && k <= MV_MAX_K, MGCR_ERR_INVALID, "mgcr_mvec_create: k = %d columns, 1 .. %d are supported", (int)k, MV_MAX_K);
    LOCK();
    mgcr_mvec_s *v = new mgcr_mvec_s();
    v->n = n;
    v->k = k;
    if (n > 0) {
        hipError_t e = hipMalloc((void **)&v->d, sizeof(cplx) * (size_t)n * (size_t)k);
        if (e != hipSuccess) {
            delete v;
            set_error("mgcr_mvec_create: hipMalloc of %lld x %d complex failed: %s", (long long)n, (int)k, hipGetErrorString(e));
            return MGCR_ERR_ALLOC;
        }
    }
    *out = v;
    return MGCR_OK;
}

int mgcr_mvec_destroy(mgcr_mvec_t v) {
    if (!v) return MGCR_OK;
    LOCK();
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    if (v->d) hipFree(v->d);
    delete v;
    return MGCR_OK;
}

int64_t mgcr_mvec_size(mgcr_mvec_t v) { return v ? v->n : -1; }
int32_t mgcr_mvec_ncols(mgcr_mvec_t v) { return v ? v->k : -1; }

int mgcr_mvec_zero(mgcr_mvec_t v) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(v, MGCR_ERR_INVALID, "mgcr_mvec_zero: null argument");
    LOCK();
    return k_zero(v->d, v->n * v->k);
}

// host [k][n] <-> device [n][k]: one copy into a staging buffer and one transposing kernel
static int mvec_transfer(mgcr_mvec_t v, double *host_ri, bool up) {
    if (v->n == 0) return MGCR_OK;
    Context &c = ctx();
    const size_t bytes = sizeof(cplx) * (size_t)v->n * (size_t)v->k;
    cplx *stage = nullptr;
    hipError_t e = hipMalloc((void **)&stage, bytes);
    if (e != hipSuccess) {
        set_error("multi-vector transfer: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return MGCR_ERR_ALLOC;
    }
    hipError_t rc = hipSuccess;
    const dim3 grid((unsigned)red_grid(v->n * v->k));
    if (up) {
        rc = hipMemcpyAsync(stage, host_ri, bytes, hipMemcpyHostToDevice, c.stream);
        if (rc == hipSuccess) {
            hipLaunchKernelGGL((mv_transpose_kernel<true>), grid, dim3(RED_THREADS), 0, c.stream, v->d, (const cplx *)stage, v->n, (int)v->k);
            rc = hipGetLastError();
        }
    } else {
        hipLaunchKernelGGL((mv_transpose_kernel<false>), grid, dim3(RED_THREADS), 0, c.stream, stage, (const cplx *)v->d, v->n, (int)v->k);
        rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipMemcpyAsync(host_ri, stage, bytes, hipMemcpyDeviceToHost, c.stream);
    }
    if (rc == hipSuccess) rc = hipStreamSynchronize(c.stream);
    hipFree(stage);
    MGCR_HIP(rc);
    return MGCR_OK;
}

int mgcr_mvec_upload(mgcr_mvec_t v, const double *host_ri) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(v && host_ri, MGCR_ERR_INVALID, "mgcr_mvec_upload: null argument");
    LOCK();
    return mvec_transfer(v, const_cast<double *>(host_ri), true);
}

int mgcr_mvec_download(mgcr_mvec_t v, double *host_ri) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(v && host_ri, MGCR_ERR_INVALID, "mgcr_mvec_download: null argument");
    LOCK();
    MGCR_TRY(mvec_transfer(v, host_ri, false));
    return resident_check();
}

int mgcr_mvec_set_column(mgcr_mvec_t v, int32_t j, mgcr_vec_t src) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(v && src, MGCR_ERR_INVALID, "mgcr_mvec_set_column: null argument");
    MGCR_CHECK(j >= 0 && j < v->k, MGCR_ERR_INVALID, "mgcr_mvec_set_column: column %d of %d", (int)j, (int)v->k);
    MGCR_CHECK(src->n == v->n, MGCR_ERR_INVALID, "Dimension mismatch. (%lld vs %lld)", (long long)v->n, (long long)src->n);
    LOCK();
    if (v->n == 0) return MGCR_OK;
    MV_LAUNCH((mv_column_kernel<true>), dim3((unsigned)red_grid(v->n)), v->d, src->d, v->n, (int)v->k, (int)j);
    return MGCR_OK;
}

int mgcr_mvec_get_column(mgcr_mvec_t v, int32_t j, mgcr_vec_t dst) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(v && dst, MGCR_ERR_INVALID, "mgcr_mvec_get_column: null argument");
    MGCR_CHECK(j >= 0 && j < v->k, MGCR_ERR_INVALID, "mgcr_mvec_get_column: column %d of %d", (int)j, (int)v->k);
    MGCR_CHECK(dst->n == v->n, MGCR_ERR_INVALID, "Dimension mismatch. (%lld vs %lld)", (long long)v->n, (long long)dst->n);
    LOCK();
    if (v->n == 0) return MGCR_OK;
    MV_LAUNCH((mv_column_kernel<false>), dim3((unsigned)red_grid(v->n)), v->d, dst->w(), v->n, (int)v->k, (int)j);
    return MGCR_OK;
}

int mgcr_mvec_dot(mgcr_mvec_t a, mgcr_mvec_t b, double *out_ri) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(a && b && out_ri, MGCR_ERR_INVALID, "mgcr_mvec_dot: null argument");
    MGCR_CHECK(a->n == b->n && a->k == b->k, MGCR_ERR_INVALID, "Lengths of two fields do not match!");
    LOCK();
    return mv_dot_to_host(a->d, b->d, a->n, a->k, out_ri);
}

int mgcr_mvec_norm2(mgcr_mvec_t a, double *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(a && out, MGCR_ERR_INVALID, "mgcr_mvec_norm2: null argument");
    LOCK();
    double r[2 * MV_MAX_K];
    MGCR_TRY(mv_dot_to_host(a->d, a->d, a->n, a->k, r));
    for (int j = 0; j < a->k; j++) out[j] = r[2 * j];
    return MGCR_OK;
}

int mgcr_mvec_axpy(const double *alpha_ri, mgcr_mvec_t x, mgcr_mvec_t y) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(x && y && alpha_ri, MGCR_ERR_INVALID, "mgcr_mvec_axpy: null argument");
    MGCR_CHECK(x->n == y->n && x->k == y->k, MGCR_ERR_INVALID, "Field dimensions do not match!");
    LOCK();
    if (x->n == 0) return MGCR_OK;
    MvAlpha al;
    for (int j = 0; j < MV_MAX_K; j++) al.a[j] = j < x->k ? make_double2(alpha_ri[2 * j], alpha_ri[2 * j + 1]) : make_double2(0., 0.);
    MV_LAUNCH_KC(mv_axpy_kernel, red_grid(x->n), x->k, al, (const cplx *)x->d, y->d, x->n, (int)x->k);
    return MGCR_OK;
}

}  // extern "C"
