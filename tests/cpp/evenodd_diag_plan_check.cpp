// Runs the even-odd host plan of a matrix with a site diagonal (csrc/evenodd_plan.h, evenodd_plan_build_diag) on the CPU:
// tests/test_evenodd_diag_plan.py builds this with g++ and the address / undefined-behaviour sanitizers, hands it a matrix in a file
// and compares what it writes with the numpy model of tests/evenodd_diag_cases.py.
//
//   evenodd_diag_plan_check IN OUT
// IN  (native int64 / double): n, nnz, has_parity; rowptr[n + 1]; col[nnz]; val[2 nnz]; parity[n] as int64 when has_parity
// OUT (on success): n_e, n_o, nnz_eo, nnz_oe; parity[n] (int64); even[n_e]; odd[n_o]; index[n];
//                   eo.rowptr[n_e + 1], eo.col, eo.val[2 nnz_eo]; oe.rowptr[n_o + 1], oe.col, oe.val[2 nnz_oe]; d[2 n]
// stdout: "OK n_e n_o n_diag"  or  "INVALID row col" followed by the message on the next line.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "evenodd_plan.h"

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
    if (argc != 3) { fprintf(stderr, "usage: evenodd_diag_plan_check IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int64_t> head, rowptr, col, par64;
    std::vector<double> val;
    bool ok = get(in, head, 3) && get(in, rowptr, (size_t)head[0] + 1) && get(in, col, (size_t)head[1]) && get(in, val, 2 * (size_t)head[1]) &&
              (!head[2] || get(in, par64, (size_t)head[0]));
    fclose(in);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    std::vector<int8_t> parity(par64.begin(), par64.end());
    mgcr::EvenOddPlan plan;
    std::string err;
    std::vector<double> d;
    int64_t n_diag = -1;
    if (!mgcr::evenodd_plan_build_diag(head[0], rowptr.data(), col.data(), val.data(), head[2] ? parity.data() : nullptr, &plan, &d, &n_diag, &err)) {
        printf("INVALID %lld %lld\n%s\n", (long long)plan.bad_row, (long long)plan.bad_col, err.c_str());
        return 0;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::vector<int64_t> sizes = {(int64_t)plan.even.size(), (int64_t)plan.odd.size(), (int64_t)plan.eo.col.size(), (int64_t)plan.oe.col.size()};
    const std::vector<int64_t> p64(plan.parity.begin(), plan.parity.end());
    ok = put(out, sizes) && put(out, p64) && put(out, plan.even) && put(out, plan.odd) && put(out, plan.index) && put(out, plan.eo.rowptr) &&
         put(out, plan.eo.col) && put(out, plan.eo.val_ri) && put(out, plan.oe.rowptr) && put(out, plan.oe.col) && put(out, plan.oe.val_ri) && put(out, d);
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "write failed\n"); return 2; }
    if (plan.eo.nrow != sizes[0] || plan.eo.ncol != sizes[1] || plan.oe.nrow != sizes[1] || plan.oe.ncol != sizes[0]) {
        fprintf(stderr, "half matrix shapes do not match the lists\n");
        return 1;
    }
    if (d.size() != 2 * (size_t)head[0]) { fprintf(stderr, "d has the wrong length\n"); return 1; }
    printf("OK %lld %lld %lld\n", (long long)sizes[0], (long long)sizes[1], (long long)n_diag);
    return 0;
}
