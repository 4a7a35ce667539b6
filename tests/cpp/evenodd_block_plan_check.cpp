// Runs the even-odd host plan of a matrix with a dense block per site (csrc/evenodd_plan.h, evenodd_plan_build_block) on the CPU:
// tests/test_evenodd_block_plan.py builds this with g++ and the address / undefined-behaviour sanitizers, hands it a matrix in a
// file and compares what it writes with the numpy model of tests/evenodd_block_cases.py.
//
//   evenodd_block_plan_check IN OUT
// IN  (native int64 / double): n, nnz, has_parity, bs; rowptr[n + 1]; col[nnz]; val[2 nnz]; parity[n] as int64 when has_parity
// OUT (on success): n_e, n_o, nnz_eo, nnz_oe; parity[n] (int64); even[n_e]; odd[n_o]; index[n];
//                   eo.rowptr[n_e + 1], eo.col, eo.val[2 nnz_eo]; oe.rowptr[n_o + 1], oe.col, oe.val[2 nnz_oe];
//                   blocks_even[2 n_e bs]; blocks_odd[2 n_o bs]
// stdout: "OK n_e n_o n_in_site"  or  "INVALID row col" followed by the message on the next line.
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
    if (argc != 3) { fprintf(stderr, "usage: evenodd_block_plan_check IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int64_t> head, rowptr, col, par64;
    std::vector<double> val;
    bool ok = get(in, head, 4) && get(in, rowptr, (size_t)head[0] + 1) && get(in, col, (size_t)head[1]) && get(in, val, 2 * (size_t)head[1]) &&
              (!head[2] || get(in, par64, (size_t)head[0]));
    fclose(in);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    std::vector<int8_t> parity(par64.begin(), par64.end());
    mgcr::EvenOddPlan plan;
    std::string err;
    std::vector<double> be, bo;
    int64_t n_in = -1;
    const int32_t bs = (int32_t)head[3];
    if (!mgcr::evenodd_plan_build_block(head[0], rowptr.data(), col.data(), val.data(), bs, head[2] ? parity.data() : nullptr, &plan, &be, &bo, &n_in,
                                        &err)) {
        printf("INVALID %lld %lld\n%s\n", (long long)plan.bad_row, (long long)plan.bad_col, err.c_str());
        return 0;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::vector<int64_t> sizes = {(int64_t)plan.even.size(), (int64_t)plan.odd.size(), (int64_t)plan.eo.col.size(), (int64_t)plan.oe.col.size()};
    const std::vector<int64_t> p64(plan.parity.begin(), plan.parity.end());
    ok = put(out, sizes) && put(out, p64) && put(out, plan.even) && put(out, plan.odd) && put(out, plan.index) && put(out, plan.eo.rowptr) &&
         put(out, plan.eo.col) && put(out, plan.eo.val_ri) && put(out, plan.oe.rowptr) && put(out, plan.oe.col) && put(out, plan.oe.val_ri) && put(out, be) && put(out, bo);
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "write failed\n"); return 2; }
    if (plan.eo.nrow != sizes[0] || plan.eo.ncol != sizes[1] || plan.oe.nrow != sizes[1] || plan.oe.ncol != sizes[0]) {
        fprintf(stderr, "half matrix shapes do not match the lists\n");
        return 1;
    }
    if (be.size() != 2 * (size_t)sizes[0] * (size_t)bs || bo.size() != 2 * (size_t)sizes[1] * (size_t)bs) {
        fprintf(stderr, "the blocks have the wrong length\n");
        return 1;
    }
    printf("OK %lld %lld %lld\n", (long long)sizes[0], (long long)sizes[1], (long long)n_in);
    return 0;
}
