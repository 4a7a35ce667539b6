// Runs the host plan of the low-precision GCR's fp32 matrix copy (csrc/gcr32_plan.h) on the CPU: tests/test_gcr32_plan.py builds this
// stand-alone program with g++ and the address / undefined-behaviour sanitizers, hands it a matrix in a file and compares what it
// writes with the numpy model of tests/gcr32_cases.py.
//
//   gcr32_plan_check IN OUT
// IN  (native int64 / double): n, nnz, tile_rows; rowptr[n + 1]; col[nnz]; val[2 nnz]
// OUT (on success, int64 / int32 / float): W, npad, real_slab, n_tail_rows, tail_nnz, n_tile_tail, stored_bytes (int64);
//                   ell_col[W npad] (int32); ell_val[W npad (x 2)] (float); tail_rows; tail_ptr; tail_col (int32); tail_val (float);
//                   tile_tail (int32)
// stdout: "OK W n_tail_rows real_slab"  or  "INVALID" followed by the message on the next line.
// A second mode checks the parameter refusals:  gcr32_plan_check param truncation restart max_iter precond use_x0 flexible profile
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gcr32_plan.h"

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
    if (argc == 9 && !strcmp(argv[1], "param")) {
        std::string err;
        const bool ok = mgcr::gcr32_param_ok(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]) != 0, atoi(argv[7]) != 0,
                                             atoi(argv[8]) != 0, &err);
        printf("%s\n%s\n", ok ? "OK" : "UNSUPPORTED", err.c_str());
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: gcr32_plan_check IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int64_t> head, rowptr, col;
    std::vector<double> val;
    bool ok = get(in, head, 3) && get(in, rowptr, (size_t)head[0] + 1) && get(in, col, (size_t)head[1]) && get(in, val, 2 * (size_t)head[1]);
    fclose(in);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    mgcr::Gcr32Plan plan;
    std::string err;
    if (!mgcr::gcr32_plan_build(head[0], rowptr.data(), col.data(), val.data(), (int32_t)head[2], &plan, &err)) {
        printf("INVALID\n%s\n", err.c_str());
        return 0;
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::vector<int64_t> sizes = {plan.W, plan.npad, plan.real_slab ? 1 : 0, (int64_t)plan.tail_rows.size(), plan.tail_nnz,
                                        (int64_t)plan.tile_tail.size(), plan.stored_bytes()};
    ok = put(out, sizes) && put(out, plan.ell_col) && put(out, plan.ell_val) && put(out, plan.tail_rows) && put(out, plan.tail_ptr) &&
         put(out, plan.tail_col) && put(out, plan.tail_val) && put(out, plan.tile_tail);
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "write failed\n"); return 2; }
    const size_t nc = plan.real_slab ? 1 : 2;
    if (plan.ell_col.size() != (size_t)plan.W * plan.npad || plan.ell_val.size() != nc * plan.ell_col.size() ||
        plan.tail_ptr.size() != plan.tail_rows.size() + 1 || plan.tail_val.size() != nc * plan.tail_col.size()) {
        fprintf(stderr, "the arrays have the wrong lengths\n");
        return 1;
    }
    printf("OK %d %lld %d\n", (int)plan.W, (long long)plan.tail_rows.size(), plan.real_slab ? 1 : 0);
    return 0;
}
