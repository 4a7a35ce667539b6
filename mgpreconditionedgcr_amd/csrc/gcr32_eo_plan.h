// Host plan of the low-precision GCR in EVEN-ODD form (gcr32_eo.hip, mgcr_gcr32_create_eo): the fp32 copy of the Schur complement
//     S = diag(a_e) - c^2 H_eo diag(1 / a_o) H_oe
// of A = diag(a) - c H (evenodd_diag.hip: Dirac form a = (1, 0) - k d, c = k; matrix form a = d, c = -1).  Pure arithmetic on plain
// data, no HIP header — tests/cpp/gcr32_eo_plan_check.cpp runs it on the CPU.
//   colouring   evenodd_plan_build_diag (evenodd_plan.h), unchanged: the rules, the check and its message are mgcr_eo_create_diag's
//   values      every stored value must be finite in float (the message names the full-system row)
//   halves      H_eo (n_e x n_o) and H_oe (n_o x n_e), each a Gcr32Plan of its own (gcr32_plan.h: its own choose_width, slab
//               [W][npad], tail, tile_tail); ONE real / complex flag for both: real when every stored off-diagonal imaginary part is 0
//   diagonal    a and 1 / a_o in fp64 by the operations of evenodd_diag.hip (diag_a, diag_inv), then (float) of real and imaginary
//               part each; c2 = (float) of c c, the product formed un-fused in fp64.  Refused: 1 / a_o exactly zero or not finite in
//               fp64 (the singular diagonal of mgcr_eo_create_diag, same words), and an a, a 1 / a_o or a c^2 that is not finite in float
//   has_diag    matrix form, or at least one stored diagonal entry — as mgcr_eo_create_diag decides; false: a = 1 / a_o = 1 are not stored
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "evenodd_plan.h"
#include "gcr32_plan.h"

namespace mgcr {

struct Gcr32EoPlan {
    EvenOddPlan eo;
    Gcr32Plan half[2];                  // [0] H_eo, [1] H_oe
    bool has_diag = false, matrix_form = false, real_slab = false;
    int64_t nnz = 0;                    // of the stored matrix, diagonal entries included
    std::vector<double> d_even, d_odd;  // d in list order, interleaved (re, im)
    int64_t stored_bytes() const {
        return half[0].stored_bytes() + half[1].stored_bytes() + (has_diag ? 8 * (int64_t)(eo.even.size() + eo.odd.size()) : 0);
    }
};

struct Gcr32EoCoef {
    std::vector<float> a_even, inv_a_odd;   // interleaved (re, im); empty without a diagonal
    float c2[2] = {0.f, 0.f};
};

// the operations of evenodd_diag.hip's diag_a and diag_inv
inline void gcr32_eo_a(const double d[2], const double k[2], bool matrix_form, double a[2]) {
    if (matrix_form) { a[0] = d[0]; a[1] = d[1]; return; }
    const double kdx = k[0] * d[0] - k[1] * d[1], kdy = k[0] * d[1] + k[1] * d[0];
    a[0] = 1. - kdx;
    a[1] = 0. - kdy;
}
inline void gcr32_eo_inv(const double a[2], double v[2]) {
    const double den = a[0] * a[0] + a[1] * a[1];
    v[0] = a[0] / den;
    v[1] = -a[1] / den;
}

// false: *err says why (MGCR_ERR_INVALID)
inline bool gcr32_eo_plan_build(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const int8_t *parity_in, bool matrix_form,
                                int32_t tile_rows, Gcr32EoPlan *out, std::string *err) {
    Gcr32EoPlan &p = *out;
    p = Gcr32EoPlan();
    std::vector<double> d;
    int64_t n_diag = 0;
    if (!evenodd_plan_build_diag(n, rowptr, col, val_ri, parity_in, &p.eo, &d, &n_diag, err)) return false;
    p.nnz = rowptr[n];
    p.matrix_form = matrix_form;
    p.has_diag = matrix_form || n_diag > 0;
    for (int64_t i = 0; i < n; i++)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; e++) {
            float re, im;
            if (!gcr32_to_float(val_ri[2 * e], &re) || !gcr32_to_float(val_ri[2 * e + 1], &im)) {
                *err = "row " + std::to_string((long long)i) + " stores a value that is not finite in single precision";
                return false;
            }
        }
    bool real = true;
    for (int h = 0; h < 2; h++) {
        const HalfCsr &H = h ? p.eo.oe : p.eo.eo;
        for (size_t e = 0; e < H.col.size(); e++)
            if (H.val_ri[2 * e + 1] != 0.) real = false;
    }
    p.real_slab = real;
    for (int h = 0; h < 2; h++) {
        const HalfCsr &H = h ? p.eo.oe : p.eo.eo;
        if (!gcr32_plan_build(H.nrow, H.rowptr.data(), H.col.data(), H.val_ri.data(), tile_rows, &p.half[h], err, H.ncol, !real)) return false;
    }
    if (p.has_diag) {
        for (int64_t r : p.eo.even) { p.d_even.push_back(d[2 * (size_t)r]); p.d_even.push_back(d[2 * (size_t)r + 1]); }
        for (int64_t r : p.eo.odd) { p.d_odd.push_back(d[2 * (size_t)r]); p.d_odd.push_back(d[2 * (size_t)r + 1]); }
    }
    return true;
}

// a_e, 1 / a_o and c^2 in float for the plan at k (k_ri is not read in matrix form); false: *err says what is refused, nothing of *out
// is to be used
inline bool gcr32_eo_coefficients(const Gcr32EoPlan &p, const double *k_ri, Gcr32EoCoef *out, std::string *err) {
    char msg[256];
    Gcr32EoCoef &c = *out;
    c = Gcr32EoCoef();
    const double one[2] = {-1., 0.};
    const double *cc = p.matrix_form ? one : k_ri;
    const double c2x = cc[0] * cc[0] - cc[1] * cc[1], c2y = cc[0] * cc[1] + cc[1] * cc[0];
    if (!gcr32_to_float(c2x, &c.c2[0]) || !gcr32_to_float(c2y, &c.c2[1])) {
        *err = "c^2 = k k is not finite in single precision";
        return false;
    }
    if (!p.has_diag) return true;
    const size_t ne = p.eo.even.size(), no = p.eo.odd.size();
    c.a_even.resize(2 * ne);
    c.inv_a_odd.resize(2 * no);
    for (size_t i = 0; i < no; i++) {   // the singular check first, as mgcr_eo_create_diag makes it
        double a[2], v[2];
        gcr32_eo_a(&p.d_odd[2 * i], cc, p.matrix_form, a);
        gcr32_eo_inv(a, v);
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || (v[0] == 0. && v[1] == 0.)) {
            snprintf(msg, sizeof msg, "the diagonal of odd row %lld has no inverse (a singular diagonal block: %s = 0 or not finite)",
                     (long long)p.eo.odd[i], p.matrix_form ? "d" : "1 - k d");
            *err = msg;
            return false;
        }
    }
    for (size_t i = 0; i < ne; i++) {
        double a[2];
        gcr32_eo_a(&p.d_even[2 * i], cc, p.matrix_form, a);
        if (!gcr32_to_float(a[0], &c.a_even[2 * i]) || !gcr32_to_float(a[1], &c.a_even[2 * i + 1])) {
            snprintf(msg, sizeof msg, "row %lld: the diagonal a is not finite in single precision", (long long)p.eo.even[i]);
            *err = msg;
            return false;
        }
    }
    for (size_t i = 0; i < no; i++) {
        double a[2], v[2];
        gcr32_eo_a(&p.d_odd[2 * i], cc, p.matrix_form, a);
        gcr32_eo_inv(a, v);
        if (!gcr32_to_float(v[0], &c.inv_a_odd[2 * i]) || !gcr32_to_float(v[1], &c.inv_a_odd[2 * i + 1])) {
            snprintf(msg, sizeof msg, "row %lld: 1 / a of the diagonal is not finite in single precision", (long long)p.eo.odd[i]);
            *err = msg;
            return false;
        }
    }
    return true;
}

}  // namespace mgcr
