// Mixed precision: (1 - k D) x = b on the 4^4 sample at k = 0.18, solved both ways — by the fp64 GCR(5) alone, and by an fp64 flexible
// GCR(5) whose right preconditioner is a LowPrecisionGCR: an fp32 copy of the matrix and 8 steps of GCR(8) in fp32 per outer step,
// run on the device without host round trips.  The outer iteration keeps the true fp64 residual, so both reach 1e-10.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/mixed_precision [matrix file] [k = 0.18]
//
// rhs init_rand(0), x0 = 0, at most 4000 steps, tolerance 1e-10.  Prints `fp64: ... after N steps`, `mixed: ... after N outer steps`,
// `one inner solve of the right-hand side: n steps, fp32 |r| / |f| = ...`, the true residual of each solution and their distance; exit status 1 if either
// solve fails to converge, a true residual exceeds 1e-9 or the two solutions differ by more than 1e-8.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <string>
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
    long dims[6] = {4, 4, 4, 4, 4, 3};
    auto D = new Sparse(read_data(file));
    if (D->get_dim() != 3072) { dims[0] = dims[1] = dims[2] = dims[3] = 8; }   // the 8x8 configuration's mesh
    DiracOp<long> A(D, std::complex<double>(k, 0.));
    Field<long> rhs(dims, 6);
    rhs.init_rand(0);

    GCR_Param<long> plain(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    GCR<long> gcr64(&A, &plain);
    Field<long> x64(rhs.get_mesh());
    x64.set_zero();
    gcr64.solve(rhs, x64);
    std::printf("fp64: %s after %d steps\n", gcr64.converged ? "converged" : "did not converge", gcr64.iterations);

    GCR_Param<long> inner(0, 8, 8, 0.1, false, nullptr, nullptr);
    LowPrecisionGCR<long> low(D, std::complex<double>(k, 0.), &inner);
    const auto info = low.info();
    std::printf("fp32 copy: %lld rows, ELL width %d, %lld tail rows, %s slab, %lld bytes\n", (long long)info.n, (int)info.ell_width, (long long)info.tail_rows,
                info.real_slab ? "real" : "complex", (long long)info.stored_bytes);
    GCR_Param<long> outer(0, 5, 4000, 1e-10, false, nullptr, &low);
    outer.flexible = true;
    GCR<long> mixed(&A, &outer);
    Field<long> x32(rhs.get_mesh());
    x32.set_zero();
    mixed.solve(rhs, x32);
    std::printf("mixed: %s after %d outer steps\n", mixed.converged ? "converged" : "did not converge", mixed.iterations);
    // one inner solve on its own (inside the solve, the last apply the outer solver enqueues is cut to 0 steps: its result is unused)
    Field<long> y = low(rhs);
    double rel = 0.;
    const int inner_steps = low.last(&rel);
    std::printf("one inner solve of the right-hand side: %d steps, fp32 |r| / |f| = %.3e\n", inner_steps, rel);

    Field<long> r64 = rhs - A(x64), r32 = rhs - A(x32), diff = x32 - x64;
    const double t64 = r64.norm() / rhs.norm(), t32 = r32.norm() / rhs.norm(), err = diff.norm() / x64.norm();
    std::printf("true residual: fp64 %.3e, mixed %.3e; |x_mixed - x_fp64| / |x_fp64| = %.3e\n", t64, t32, err);
    const bool ok = gcr64.converged && mixed.converged && t64 <= 1e-9 && t32 <= 1e-9 && err <= 1e-8;
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete D;
    return ok ? 0 : 1;
}
