// Runs the host plan of the low-precision GCR in even-odd form (csrc/gcr32_eo_plan.h) on the CPU: tests/test_gcr32_eo_plan.py builds
// this stand-alone program with g++ and the address / undefined-behaviour sanitizers, hands it a matrix in a file and compares what it
// writes with the numpy model of tests/gcr32_eo_cases.py.
//
//   gcr32_eo_plan_check IN OUT
// IN  (native int64 / double / int8): n, nnz, tile_rows, has_parity, matrix_form; k[2] (double); rowptr[n + 1]; col[nnz]; val[2 nnz];
//                   parity[n] when has_parity
// OUT (on success): n_e, n_o, has_diag, real_slab, stored_bytes (int64); parity[n] (int8); c2[2] (float);
//                   a_even[2 n_e], inv_a_odd[2 n_o] (float, when has_diag); then for H_eo and for H_oe:
//                   W, npad, n_tail_rows, tail_nnz, n_tile_tail (int64); ell_col; ell_val; tail_rows; tail_ptr; tail_col; tail_val; tile_tail
// stdout: "OK n_e n_o has_diag real_slab"  or  "INVALID" followed by the message on the next line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gcr32_eo_plan.h"

template <typename T>
static bool get(FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <typename T>
static bool put(FILE *f, const std::vector<T> &v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: gcr32_eo_plan_check IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int64_t> head, rowptr, col;
    std::vector<double> k, val;
    std::vector<int8_t> parity;
    bool ok = get(in, head, 5) && get(in, k, 2) && get(in, rowptr, (size_t)head[0] + 1) && get(in, col, (size_t)head[1]) &&
              get(in, val, 2 * (size_t)head[1]) && get(in, parity, head[3] ? (size_t)head[0] : 0);
    fclose(in);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    const bool matrix_form = head[4] != 0;
    mgcr::Gcr32EoPlan plan;
    mgcr::Gcr32EoCoef co;
    std::string err;
    if (!mgcr::gcr32_eo_plan_build(head[0], rowptr.data(), col.data(), val.data(), head[3] ? parity.data() : nullptr, matrix_form, (int32_t)head[2],
                                   &plan, &err) ||
        !mgcr::gcr32_eo_coefficients(plan, matrix_form ? nullptr : k.data(), &co, &err)) {
        printf("INVALID\n%s\n", err.c_str());
        return 0;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const int64_t ne = (int64_t)plan.eo.even.size(), no = (int64_t)plan.eo.odd.size();
    const std::vector<int64_t> sizes = {ne, no, plan.has_diag ? 1 : 0, plan.real_slab ? 1 : 0, plan.stored_bytes()};
    const std::vector<float> c2 = {co.c2[0], co.c2[1]};
    ok = put(out, sizes) && put(out, plan.eo.parity) && put(out, c2) && put(out, co.a_even) && put(out, co.inv_a_odd);
    for (int h = 0; h < 2 && ok; h++) {
        const mgcr::Gcr32Plan &p = plan.half[h];
        const std::vector<int64_t> hs = {p.W, p.npad, (int64_t)p.tail_rows.size(), p.tail_nnz, (int64_t)p.tile_tail.size()};
        ok = put(out, hs) && put(out, p.ell_col) && put(out, p.ell_val) && put(out, p.tail_rows) && put(out, p.tail_ptr) && put(out, p.tail_col) &&
             put(out, p.tail_val) && put(out, p.tile_tail);
        const size_t nc = plan.real_slab ? 1 : 2;
        if (p.real_slab != plan.real_slab || p.ell_col.size() != (size_t)p.W * p.npad || p.ell_val.size() != nc * p.ell_col.size() ||
            p.tail_ptr.size() != p.tail_rows.size() + 1 || p.tail_val.size() != nc * p.tail_col.size()) {
            fprintf(stderr, "the arrays of half %d have the wrong lengths or the wrong slab kind\n", h);
            return 1;
        }
    }
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "write failed\n"); return 2; }
    if (plan.has_diag && (co.a_even.size() != 2 * (size_t)ne || co.inv_a_odd.size() != 2 * (size_t)no)) {
        fprintf(stderr, "the diagonals have the wrong lengths\n");
        return 1;
    }
    printf("OK %lld %lld %d %d\n", (long long)ne, (long long)no, plan.has_diag ? 1 : 0, plan.real_slab ? 1 : 0);
    return 0;
}
