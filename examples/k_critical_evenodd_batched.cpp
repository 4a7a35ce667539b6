// An even-odd hopping-parameter scan as ONE batched solve: (1 - k_j D) x_j = b for a list of k_j, every column solved as its Schur
// system on the even half of the lattice, S_j x_e = b_e + k_j D_eo b_o with S_j = 1 - k_j^2 D_eo D_oe, and x_o reconstructed
// (MultiEvenOddDiracOp::solve).  examples/k_critical_evenodd.cpp walks the same ladder one k at a time, examples/k_critical_batched.cpp
// batches the full systems; here the two halves of D are streamed once per step for the whole ladder AND every Krylov vector is
// half as long.  A column that has converged is frozen while the others go on.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/k_critical_evenodd_batched [matrix file] k_1 [k_2 ...]
//
// k_j: `re` or `re,im`; at most 16 of them.  GCR(5), at most 4000 steps, tolerance 1e-10, rhs init_rand(0), x0 = 0.
// Prints the lines of k_critical_evenodd: per k, `[j] Step i residual norm = ...` (the Schur solve's history, relative to
// |b_e + k_j D_eo b_o|) and `k = ...: converged / did not converge after N steps, |x|^2 = ...` for the reconstructed full solution.
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
    std::vector<std::complex<double>> ks;
    for (int a = 1; a < argc; a++) {
        char *end = nullptr, *end2 = nullptr;
        const double re = std::strtod(argv[a], &end);
        const double im = end != argv[a] && *end == ',' ? std::strtod(end + 1, &end2) : 0.;
        if (end == argv[a] || (*end != '\0' && !(*end == ',' && end2 != end + 1 && *end2 == '\0'))) {   // not a number: the matrix file
            file = argv[a];
            continue;
        }
        ks.push_back(std::complex<double>(re, im));
    }
    if (ks.empty() || ks.size() > 16) {
        std::fprintf(stderr, "usage: %s [matrix file] k_1 [k_2 ... k_16]   (k_j: re or re,im)\n", argv[0]);
        return 2;
    }
    long dims[6] = {4, 4, 4, 4, 4, 3};
    auto D = new Sparse(read_data(file));
    if (D->get_dim() != 3072) { dims[0] = dims[1] = dims[2] = dims[3] = 8; }   // the 8x8 configuration's mesh

    Field<long> rhs(dims, 6);
    rhs.init_rand(0);
    GCR_Param<long> param(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    EvenOddDiracOp<long> eo(D, ks[0]);           // the rows are two-coloured once; its own k is not used below
    std::printf("even-odd: %ld rows, %ld even, %ld odd\n", eo.get_n(), eo.get_n_even(), eo.get_n_odd());
    const int k = (int)ks.size();
    {
        MultiEvenOddDiracOp<long> scan(&eo, ks);
        MultiField<long> B(std::vector<const Field<long> *>((size_t)k, &rhs));
        MultiField<long> X(rhs.get_mesh(), k);
        X.set_zero();
        scan.solve(B, X, &param);                // ONE solve for the whole ladder
        const std::vector<double> x2 = X.squarednorm();
        for (int j = 0; j < k; j++) {
            for (int i = 0; i <= scan.last_iterations[(size_t)j]; i++)
                std::printf("[%d] Step %d residual norm = %.10e\n", j, i, scan.last_history[(size_t)j][(size_t)i]);
            char name[64];
            if (ks[(size_t)j].imag() != 0.) std::snprintf(name, sizeof name, "%g%+gi", ks[(size_t)j].real(), ks[(size_t)j].imag());
            else std::snprintf(name, sizeof name, "%g", ks[(size_t)j].real());
            std::printf("k = %s: %s after %d steps, |x|^2 = %.10e\n", name, scan.last_converged[(size_t)j] ? "converged" : "did not converge",
                        scan.last_iterations[(size_t)j], x2[(size_t)j]);
        }
    }
    delete D;
    return 0;
}
