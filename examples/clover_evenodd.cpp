// The even-odd Schur solve of a clover-type operator: A = 1 - k (D + C), D the sample hopping matrix (256 sites of 12 spin-colour
// rows) and C a seeded Hermitian 12 x 12 block on every site, through EvenOddBlockDiracOp — the Dirac form of mgcr_eo_create_block
// with bs = 12.  The Schur system on the even sites, S x_e = b_e + k D_eo (B_o^-1 b_o) with S = B_e - k^2 D_eo B_o^-1 D_oe and
// B_s = I - k C_s, is solved by GCR(5) and the odd half reconstructed; the result is checked against the full DiracOp solve of the
// same matrix.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/clover_evenodd [matrix file] [scale = 1]
//
// C_s = scale (G_s + G_s^H) / 2 with G_s[i][j] = ((7919 q) mod 1013) / 1013 - 1/2 + i (((104729 q) mod 997) / 997 - 1/2),
// q = (12 s + i) 12 + j + 1; a row stores its 12 block entries first, then its hops.  k = 0.15,
// rhs_i = ((7919 i) mod 1013) / 1013 - 1/2 + i (((104729 i) mod 997) / 997 - 1/2), x0 = 0, at most 4000 steps, tolerance 1e-8.
// Prints `even-odd: N rows, n_e even, n_o odd, bs = 12`, the Schur solve's history as `Step i residual norm = ...` (relative to
// |bhat_e|), `schur: ... after N steps, |x|^2 = ...`, `full: ... after N steps`, the distance of the two solutions and the true
// residual of the even-odd one; exit status 1 if they disagree.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "Fields.h"
#include "GCR.h"
#include "Parse.h"
#include "Operator.h"

typedef std::complex<double> cd;
static const long BS = 12;

static cd seeded(long q) { return cd((double)((7919 * q) % 1013) / 1013. - 0.5, (double)((104729 * q) % 997) / 997. - 0.5); }
static cd clover(long s, long i, long j, double scale) {
    const cd a = seeded((BS * s + i) * BS + j + 1), b = seeded((BS * s + j) * BS + i + 1);
    return scale * (a + std::conj(b)) / 2.;
}

int main(int argc, char **argv) {
    std::string file = "4x4parsed.txt";
    double scale = 1.;
    bool bad = argc > 3;
    for (int a = 1; a < argc && !bad; a++) {
        char *end = nullptr;
        const double v = std::strtod(argv[a], &end);
        if (end != argv[a] && *end == '\0') { scale = v; bad = !(v >= 0.) || !std::isfinite(v); }
        else if (a == 1) file = argv[a];
        else bad = true;
    }
    if (bad) {
        std::fprintf(stderr, "usage: %s [matrix file] [scale = 1]   (scale >= 0)\n", argv[0]);
        return 2;
    }
    Sparse<long> *D = new Sparse<long>(read_data(file));
    const long N = D->get_nrow(), nnz = D->get_nnz();
    if (N != D->get_dim() || N % BS != 0) { std::fprintf(stderr, "the matrix must be square with a multiple of 12 rows\n"); return 2; }
    Sparse<long> *M = new Sparse<long>(N, N, nnz + N * BS);      // D + C
    long p = 0;
    for (long r = 0; r < N; r++) {
        M->mod_ROW_at(r, p);
        const long s = r / BS;
        for (long j = 0; j < BS; j++, p++) { M->mod_COL_at(p, s * BS + j); M->mod_VAL_at(p, clover(s, r % BS, j, scale)); }
        for (long e = D->get_ROW(r); e < D->get_ROW(r + 1); e++, p++) { M->mod_COL_at(p, D->get_COL(e)); M->mod_VAL_at(p, D->val_at(e)); }
    }
    M->mod_ROW_at(N, p);
    delete D;

    long dims[1] = {N};
    Field<long> rhs(dims, 1);
    for (long i = 0; i < N; i++) rhs.mod_val_at(i, seeded(i));
    const cd k(0.15, 0.);
    GCR_Param<long> param(0, 5, 4000, 1e-8, false, nullptr, nullptr);
    EvenOddBlockDiracOp<long> eo(M, k, (int)BS);
    std::printf("even-odd: %ld rows, %ld even, %ld odd, bs = %ld\n", eo.get_n(), eo.get_n_even(), eo.get_n_odd(), BS);
    Field<long> x(dims, 1);
    x.set_zero();
    eo.solve(rhs, x, &param);
    for (int i = 0; i <= eo.last_iterations; i++) std::printf("Step %d residual norm = %.10e\n", i, eo.last_history[(size_t)i]);
    std::printf("schur: %s after %d steps, |x|^2 = %.10e\n", eo.last_converged ? "converged" : "did not converge", eo.last_iterations, x.squarednorm());

    DiracOp<long> A(M, k);
    Field<long> xf(dims, 1);
    xf.set_zero();
    GCR<long> gcr(&A, &param);
    gcr.solve(rhs, xf);
    const int full_steps = (int)gcr.history.size() - 1;
    std::printf("full: %s after %d steps\n", gcr.history.back() <= 1e-8 ? "converged" : "did not converge", full_steps);
    Field<long> diff = x - xf, r = rhs - A(x);
    const double err = diff.norm() / xf.norm(), res = r.norm() / rhs.norm();
    std::printf("|x_schur - x_full| / |x_full| = %.3e, true residual of the even-odd solution = %.3e\n", err, res);
    const bool ok = eo.last_converged && gcr.history.back() <= 1e-8 && err <= 1e-5 && res <= 1e-7 && eo.last_iterations < full_steps;
    std::printf("%s\n", ok ? "OK" : "MISMATCH");
    delete M;
    return ok ? 0 : 1;
}
