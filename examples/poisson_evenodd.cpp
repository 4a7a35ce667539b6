// The even-odd Schur solve of a matrix that stores its diagonal: the 7-point Poisson matrix of an nx x ny x nz box (6 on the
// diagonal, -1 off it, open boundaries), red-black ordered by EvenOddSparse — the matrix form of mgcr_eo_create_diag.  The Schur
// system on the even sites, S x_e = b_e + M_eo (b_o / d_o) with S = diag(d_e) - M_eo diag(1/d_o) M_oe, is solved by GCR(5) and the
// odd half reconstructed; the result is checked against the full solve of M x = b.
//
//   make -C examples
//   examples/build/poisson_evenodd [nx = 6] [ny = 5] [nz = 4]
//
// rhs_i = ((7919 i) mod 1013) / 1013 - 1/2 + i (((104729 i) mod 997) / 997 - 1/2), x0 = 0, at most 4000 steps, tolerance 1e-10.
// Prints `even-odd: N rows, n_e even, n_o odd`, the Schur solve's history as `Step i residual norm = ...` (relative to |bhat_e|),
// `schur: ... after N steps, |x|^2 = ...`, `full: ... after N steps`, the distance of the two solutions and the true residual of the
// even-odd one; exit status 1 if they disagree.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "Fields.h"
#include "GCR.h"
#include "Operator.h"

static Sparse<long> *poisson_box(long nx, long ny, long nz) {
    const long N = nx * ny * nz;
    long nnz = 0;
    for (long i = 0; i < nx; i++)
        for (long j = 0; j < ny; j++)
            for (long k = 0; k < nz; k++) nnz += 1 + (i > 0) + (i < nx - 1) + (j > 0) + (j < ny - 1) + (k > 0) + (k < nz - 1);
    auto *A = new Sparse<long>(N, N, nnz);
    long p = 0;
    for (long i = 0; i < nx; i++)
        for (long j = 0; j < ny; j++)
            for (long k = 0; k < nz; k++) {
                const long row = (i * ny + j) * nz + k;
                A->mod_ROW_at(row, p);
                auto put = [&](bool in, long col, double v) { if (in) { A->mod_COL_at(p, col); A->mod_VAL_at(p, std::complex<double>(v, 0.)); p++; } };
                put(i > 0, row - ny * nz, -1.); put(j > 0, row - nz, -1.); put(k > 0, row - 1, -1.);
                put(true, row, 6.);
                put(k < nz - 1, row + 1, -1.); put(j < ny - 1, row + nz, -1.); put(i < nx - 1, row + ny * nz, -1.);
            }
    A->mod_ROW_at(N, p);
    return A;
}

int main(int argc, char **argv) {
    const long nx = argc > 1 ? std::atol(argv[1]) : 6, ny = argc > 2 ? std::atol(argv[2]) : 5, nz = argc > 3 ? std::atol(argv[3]) : 4;
    if (nx < 1 || ny < 1 || nz < 1 || argc > 4) {
        std::fprintf(stderr, "usage: %s [nx = 6] [ny = 5] [nz = 4]\n", argv[0]);
        return 2;
    }
    long dims[3] = {nx, ny, nz};
    const long N = nx * ny * nz;
    Sparse<long> *A = poisson_box(nx, ny, nz);
    Field<long> rhs(dims, 3);
    for (long i = 0; i < N; i++)
        rhs.mod_val_at(i, std::complex<double>((double)((7919 * i) % 1013) / 1013. - 0.5, (double)((104729 * i) % 997) / 997. - 0.5));

    GCR_Param<long> param(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    EvenOddSparse<long> eo(A);
    std::printf("even-odd: %ld rows, %ld even, %ld odd\n", eo.get_n(), eo.get_n_even(), eo.get_n_odd());
    Field<long> x(dims, 3);
    x.set_zero();
    eo.solve(rhs, x, &param);
    for (int i = 0; i <= eo.last_iterations; i++) std::printf("Step %d residual norm = %.10e\n", i, eo.last_history[(size_t)i]);
    std::printf("schur: %s after %d steps, |x|^2 = %.10e\n", eo.last_converged ? "converged" : "did not converge", eo.last_iterations, x.squarednorm());

    Field<long> xf(dims, 3);
    xf.set_zero();
    GCR<long> gcr(A, &param);
    gcr.solve(rhs, xf);
    const int full_steps = (int)gcr.history.size() - 1;
    std::printf("full: %s after %d steps\n", gcr.history.back() <= 1e-10 ? "converged" : "did not converge", full_steps);
    Field<long> diff = x - xf, r = rhs - (*A)(x);
    const double err = diff.norm() / xf.norm(), res = r.norm() / rhs.norm();
    std::printf("|x_schur - x_full| / |x_full| = %.3e, true residual of the even-odd solution = %.3e\n", err, res);
    const bool ok = eo.last_converged && gcr.history.back() <= 1e-10 && err <= 1e-8 && res <= 1e-9 && eo.last_iterations < full_steps;
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete A;
    return ok ? 0 : 1;
}
