// Batched mixed precision: (1 - k D) X = B on the 4^4 sample at k = 0.18 for a block of 4 right-hand sides, by fp64 defect correction
// around the k-wide fp32 inner solve (LowPrecisionGCR::solve_multi): R = B - A X, X += inner_multi(R), the 4 inner solves advancing in
// lockstep — 8 steps of GCR(8) in fp32 per outer step, the fp32 matrix streamed once per step for all 4 columns.  The outer
// iteration keeps the true fp64 residual, so every column reaches 1e-10.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/mixed_precision_batched [matrix file] [k = 0.18]
//
// rhs init_rand(j) for column j, x0 = 0, at most 60 outer steps, tolerance 1e-10.  Prints per column `column j: converged after N outer
// steps, true residual ...` and the distance to the single mixed solve of that column; exit status 1 if a column fails to converge, a
// true residual exceeds 1e-9 or a column differs from its single solve by more than 1e-8.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "Fields.h"
#include "GCR.h"
#include "Parse.h"
#include "Operator.h"

int main(int argc, char **argv) {
    std::string file = "4x4parsed.txt";
    double k = 0.18;
    for (int a = 1; a < argc; a++) {
        char *end = nullptr;
        const double v = std::strtod(argv[a], &end);
        if (end == argv[a] || *end != '\0') file = argv[a];
        else k = v;
    }
    const int ncols = 4;
    long dims[6] = {4, 4, 4, 4, 4, 3};
    auto D = new Sparse(read_data(file));
    if (D->get_dim() != 3072) { dims[0] = dims[1] = dims[2] = dims[3] = 8; }   // the 8x8 configuration's mesh
    DiracOp<long> A(D, std::complex<double>(k, 0.));
    std::vector<Field<long>> rhs;
    for (int j = 0; j < ncols; j++) {
        rhs.emplace_back(dims, 6);
        rhs.back().init_rand(j);
    }
    MultiField<long> B(rhs), X(rhs[0].get_mesh(), ncols);
    X.set_zero();

    GCR_Param<long> inner(0, 8, 8, 0.1, false, nullptr, nullptr);
    LowPrecisionGCR<long> low(D, std::complex<double>(k, 0.), &inner);
    low.solve_multi(A, B, X, 1e-10, 60);
    std::vector<double> rel;
    const std::vector<int> steps = low.last_multi(&rel);

    // the single mixed solve of every column, for comparison: the fp64 flexible GCR(5) with the same operator in its right_precond slot
    GCR_Param<long> outer(0, 5, 4000, 1e-10, false, nullptr, &low);
    outer.flexible = true;
    GCR<long> mixed(&A, &outer);
    bool ok = true;
    for (int j = 0; j < ncols; j++) {
        Field<long> xj = X.column(j), xs(rhs[(size_t)j].get_mesh());
        xs.set_zero();
        mixed.solve(rhs[(size_t)j], xs);
        Field<long> r = rhs[(size_t)j] - A(xj), diff = xj - xs;
        const double t = r.norm() / rhs[(size_t)j].norm(), err = diff.norm() / xs.norm();
        std::printf("column %d: %s after %d outer steps, true residual %.3e; last inner solve %d steps, fp32 |r| / |f| = %.3e; "
                    "|x - x_single| / |x_single| = %.3e (single: %d outer steps)\n",
                    j, low.last_converged[(size_t)j] ? "converged" : "did not converge", low.last_iterations[(size_t)j], t, steps[(size_t)j], rel[(size_t)j], err,
                    mixed.iterations);
        ok = ok && low.last_converged[(size_t)j] && mixed.converged && t <= 1e-9 && err <= 1e-8;
    }
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete D;
    return ok ? 0 : 1;
}
