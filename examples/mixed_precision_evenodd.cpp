// Mixed precision on the even-odd Schur system: (1 - k D) x = b on the 4^4 sample at k = 0.18, solved through EvenOddDiracOp::solve
// both ways — the fp64 GCR(5) on the Schur system alone, and the same solve with a LowPrecisionEvenOddGCR as flexible right
// preconditioner: an fp32 copy of the Schur complement and 8 steps of GCR(8) in fp32 per outer step, run on the device without host
// round trips.  The outer iteration keeps the true fp64 residual, so both reach 1e-10.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/mixed_precision_evenodd [matrix file] [k = 0.18]
//
// rhs init_rand(0), x0 = 0, at most 4000 steps, tolerance 1e-10.  Prints `even-odd fp64: ... after N steps`, `even-odd mixed: ... after
// N outer steps`, the fp32 copy's layout, the full system's true residual of each solution and their distance; exit status 1 if either
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
    EvenOddDiracOp<long> S(D, std::complex<double>(k, 0.));
    Field<long> rhs(dims, 6);
    rhs.init_rand(0);

    GCR_Param<long> plain(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    Field<long> x64(rhs.get_mesh());
    x64.set_zero();
    S.solve(rhs, x64, &plain);
    const bool conv64 = S.last_converged;
    std::printf("even-odd fp64: %s after %d steps\n", conv64 ? "converged" : "did not converge", S.last_iterations);

    GCR_Param<long> inner(0, 8, 8, 0.1, false, nullptr, nullptr);
    LowPrecisionEvenOddGCR<long> low(D, std::complex<double>(k, 0.), &inner);
    const auto info = low.eo_info();
    std::printf("fp32 Schur copy: %lld rows (%lld even, %lld odd), widths %d / %d, %lld / %lld tail rows, %s slab, %s, %lld bytes\n", (long long)info.n,
                (long long)info.n_even, (long long)info.n_odd, (int)info.width_eo, (int)info.width_oe, (long long)info.tail_rows_eo,
                (long long)info.tail_rows_oe, info.real_slab ? "real" : "complex", info.has_diag ? "site diagonal" : "no diagonal",
                (long long)info.stored_bytes);
    GCR_Param<long> outer(0, 5, 4000, 1e-10, false, nullptr, &low);
    outer.flexible = true;
    Field<long> x32(rhs.get_mesh());
    x32.set_zero();
    S.solve(rhs, x32, &outer);
    const bool conv32 = S.last_converged;
    std::printf("even-odd mixed: %s after %d outer steps\n", conv32 ? "converged" : "did not converge", S.last_iterations);

    Field<long> r64 = rhs - A(x64), r32 = rhs - A(x32), diff = x32 - x64;
    const double t64 = r64.norm() / rhs.norm(), t32 = r32.norm() / rhs.norm(), err = diff.norm() / x64.norm();
    std::printf("true residual of the full system: fp64 %.3e, mixed %.3e; |x_mixed - x_fp64| / |x_fp64| = %.3e\n", t64, t32, err);
    const bool ok = conv64 && conv32 && t64 <= 1e-9 && t32 <= 1e-9 && err <= 1e-8;
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete D;
    return ok ? 0 : 1;
}
