// Host decisions of the low-precision GCR's fp32 matrix copy (gcr32.hip) that are pure arithmetic: plain data in, plain data out,
// no HIP header — tests/cpp/gcr32_plan_check.cpp runs them on the CPU.
//   values   (float)re, (float)im, round to nearest; a value that is not finite, or that rounds to an infinity, refuses the matrix
//            and the message names the row
//   slab     real (4 B per value) when every stored imaginary part is zero, else complex (8 B)
//   layout   W = choose_width (spmv_layout.h, the plain Sparse slab's pick), one thread per row, int32 columns, column-major
//            slab [W][npad] (entry w of row i at w * npad + i, padding: column -1), rows longer than W keep entries W .. in a CSR tail;
//            tile_tail[t] = first tail row (index into tail_rows) at or behind row t * tile_rows: a workgroup looks its tile's few tail
//            rows up there
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "spmv_layout.h"

namespace mgcr {

struct Gcr32Plan {
    int64_t n = 0, npad = 0, nnz = 0, tail_nnz = 0;
    int32_t W = 0;
    bool real_slab = false;
    std::vector<float> ell_val;      // [W][npad] (real slab) or [W][npad][2]
    std::vector<int32_t> ell_col;    // [W][npad], -1: padding
    std::vector<int32_t> tail_rows;  // ascending
    std::vector<int32_t> tail_ptr;   // [tail_rows + 1]
    std::vector<int32_t> tail_col;
    std::vector<float> tail_val;     // [tail_nnz] or [tail_nnz][2]
    std::vector<int32_t> tile_tail;  // [ntiles + 1]
    int64_t stored_bytes() const {
        const int64_t vb = real_slab ? 4 : 8;
        return (int64_t)W * npad * (4 + vb) + tail_nnz * (4 + vb) + (int64_t)tail_rows.size() * 8 + (int64_t)tile_tail.size() * 4;
    }
};

// (float)v with the overflow check: false when v is not finite or becomes infinite
inline bool gcr32_to_float(double v, float *out) {
    const float f = (float)v;
    *out = f;
    return std::isfinite(v) && std::isfinite(f);
}

// false: *err says why (inconsistent CSR, non-square, a value out of float's range).  ncol: the column count of a rectangular
// matrix — a half of the even-odd form (gcr32_eo_plan.h) —, default: square; force_complex: a complex slab whatever the values
// (the two halves of one operator share one kernel form)
inline bool gcr32_plan_build(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, int32_t tile_rows, Gcr32Plan *out,
                             std::string *err, int64_t ncol = -1, bool force_complex = false) {
    Gcr32Plan &p = *out;
    p = Gcr32Plan();
    const bool square = ncol < 0;
    if (square) ncol = n;
    if (n < 0 || n >= ((int64_t)1 << 31) || ncol >= ((int64_t)1 << 31)) { *err = "the dimension must fit int32 (got " + std::to_string((long long)(n > ncol ? n : ncol)) + ")"; return false; }
    if (rowptr[0] != 0) { *err = "inconsistent CSR: rowptr[0] != 0"; return false; }
    int64_t maxlen = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t len = rowptr[i + 1] - rowptr[i];
        if (len < 0) { *err = "inconsistent CSR: rowptr decreases at row " + std::to_string((long long)i); return false; }
        if (len > maxlen) maxlen = len;
    }
    const int64_t nnz = rowptr[n];
    if (nnz >= ((int64_t)1 << 31) || maxlen >= ((int64_t)1 << 30)) { *err = "the entry count must fit int32"; return false; }
    bool real = !force_complex;
    for (int64_t i = 0; i < n; i++)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++) {
            if (col[e] < 0 || col[e] >= ncol) {
                *err = "row " + std::to_string((long long)i) + " has column " + std::to_string((long long)col[e]) + ": the matrix must be " +
                       (square ? "square, " : "") + std::to_string((long long)n) + " x " + std::to_string((long long)ncol);
                return false;
            }
            float re, im;
            if (!gcr32_to_float(val_ri[2 * e], &re) || !gcr32_to_float(val_ri[2 * e + 1], &im)) {
                *err = "row " + std::to_string((long long)i) + " stores a value that is not finite in single precision";
                return false;
            }
            if (val_ri[2 * e + 1] != 0.) real = false;
        }
    std::vector<int64_t> hist((size_t)maxlen + 1, 0);
    for (int64_t i = 0; i < n; i++) hist[(size_t)(rowptr[i + 1] - rowptr[i])]++;
    p.n = n; p.nnz = nnz; p.real_slab = real;
    p.W = n > 0 ? choose_width(hist, n, (int32_t)maxlen) : 0;
    p.npad = (n + 63) / 64 * 64;
    const int W = p.W, nc = real ? 1 : 2;
    p.ell_val.assign((size_t)W * p.npad * nc, 0.f);
    p.ell_col.assign((size_t)W * p.npad, -1);
    p.tail_ptr.push_back(0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t e0 = rowptr[i], len = rowptr[i + 1] - e0;
        for (int64_t w = 0; w < len; w++) {
            const float re = (float)val_ri[2 * (e0 + w)], im = (float)val_ri[2 * (e0 + w) + 1];
            if (w < W) {
                const size_t at = (size_t)w * p.npad + i;
                p.ell_col[at] = (int32_t)col[e0 + w];
                if (real) p.ell_val[at] = re;
                else { p.ell_val[2 * at] = re; p.ell_val[2 * at + 1] = im; }
            } else {
                p.tail_col.push_back((int32_t)col[e0 + w]);
                p.tail_val.push_back(re);
                if (!real) p.tail_val.push_back(im);
            }
        }
        if (len > W) {
            p.tail_rows.push_back((int32_t)i);
            p.tail_ptr.push_back((int32_t)p.tail_col.size());
        }
    }
    p.tail_nnz = (int64_t)p.tail_col.size();
    const int64_t ntiles = (n + tile_rows - 1) / tile_rows;
    p.tile_tail.assign((size_t)ntiles + 1, (int32_t)p.tail_rows.size());
    for (int32_t t = (int32_t)p.tail_rows.size() - 1; t >= 0; t--) p.tile_tail[(size_t)(p.tail_rows[(size_t)t] / tile_rows)] = t;
    for (int64_t q = ntiles - 1; q >= 0; q--)
        if (p.tile_tail[(size_t)q] > p.tile_tail[(size_t)q + 1]) p.tile_tail[(size_t)q] = p.tile_tail[(size_t)q + 1];
    return true;
}

// the inner parameters the operator takes; false: *err names what it refuses (MGCR_ERR_UNSUPPORTED)
constexpr int GCR32_MAX_RESTART = 16;
inline bool gcr32_param_ok(int truncation, int restart, int max_iter, bool has_precond, bool use_x0, bool flexible, bool profile_spmv,
                           std::string *err) {
    if (truncation != 0) { *err = "truncation mode is not supported (restart mode only)"; return false; }
    if (restart < 1 || restart > GCR32_MAX_RESTART) { *err = "restart = " + std::to_string(restart) + ", 1 .. 16 slots are supported"; return false; }
    if (has_precond) { *err = "the inner solve takes no preconditioner"; return false; }
    if (use_x0 || flexible || profile_spmv) { *err = "use_x0, flexible and profile_spmv are not supported in the inner parameters"; return false; }
    (void)max_iter;
    return true;
}

}  // namespace mgcr
