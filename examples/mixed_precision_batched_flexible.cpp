// Flexible batched GCR: (1 - k D) X = B on the 4^4 sample at k = 0.18 for a block of 4 right-hand sides, by ONE batched fp64 GCR(5)
// whose flexible right preconditioner is the k-wide fp32 inner solve (GCR::solve_multi with GCR_Param::right_precond = a
// LowPrecisionGCR, flexible = true): per outer step the 4 inner solves advance in lockstep — 8 steps of GCR(8) in fp32, the fp32
// matrix streamed once per step for all 4 columns — and every column has the bits of the single mixed solve on that column alone.
// Beside it the batched defect correction around the same inner solve (LowPrecisionGCR::solve_multi).  An outer GCR accelerates over
// its cycle where the stationary defect correction only contracts: on ill-conditioned operators use this solve.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/mixed_precision_batched_flexible [matrix file] [k = 0.18]
//
// rhs init_rand(j) for column j, x0 = 0, tolerance 1e-10.  Prints per column the outer steps of the flexible batched solve, of the
// single mixed solve and of the defect correction, and the true residual; exit status 1 if a column fails to converge, a true
// residual exceeds 1e-9, or a column's step count or x differs from its single mixed solve.
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
    MultiField<long> B(rhs), X(rhs[0].get_mesh(), ncols), XD(rhs[0].get_mesh(), ncols);
    X.set_zero();
    XD.set_zero();

    GCR_Param<long> inner(0, 8, 8, 0.1, false, nullptr, nullptr);
    LowPrecisionGCR<long> low(D, std::complex<double>(k, 0.), &inner);
    GCR_Param<long> outer(0, 5, 400, 1e-10, false, nullptr, &low);
    outer.flexible = true;
    GCR<long> mixed(&A, &outer);
    mixed.solve_multi(B, X);                       // (F) the flexible batched GCR
    const std::vector<int> flex_steps = mixed.last_iterations;
    const std::vector<bool> flex_conv = mixed.last_converged;
    low.solve_multi(A, B, XD, 1e-10, 60);          // (E) defect correction around the same inner solve

    bool ok = true;
    for (int j = 0; j < ncols; j++) {
        Field<long> xj = X.column(j), xs(rhs[(size_t)j].get_mesh());
        xs.set_zero();
        mixed.solve(rhs[(size_t)j], xs);           // (A) the single mixed solve of the column
        Field<long> r = rhs[(size_t)j] - A(xj), diff = xj - xs;
        const double t = r.norm() / rhs[(size_t)j].norm(), err = diff.norm();
        std::printf("column %d: flexible batched GCR %s after %d outer steps (single mixed solve: %d, defect correction: %d), true residual %.3e, "
                    "|x - x_single| = %.1e\n",
                    j, flex_conv[(size_t)j] ? "converged" : "did not converge", flex_steps[(size_t)j], mixed.iterations, low.last_iterations[(size_t)j], t, err);
        ok = ok && flex_conv[(size_t)j] && mixed.converged && t <= 1e-9 && flex_steps[(size_t)j] == mixed.iterations && err == 0.;
    }
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete D;
    return ok ? 0 : 1;
}
