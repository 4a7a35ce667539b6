// A hopping-parameter scan through the even-odd preconditioned operator: (1 - k_j D) x_j = b solved as the Schur system on the even
// half of the lattice, S x_e = b_e + k D_eo b_o with S = 1 - k^2 D_eo D_oe, and x_o reconstructed (EvenOddDiracOp::solve;
// examples/k_critical_queue.cpp is the full-system form).  Every Krylov vector is half as long and the solve takes fewer steps.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/k_critical_evenodd [matrix file] k_1 [k_2 ...]
//
// k_j: `re` or `re,im`.  GCR(5), at most 4000 steps, tolerance 1e-10, rhs init_rand(0), x0 = 0.
// Prints, per k, `[j] Step i residual norm = ...` (the Schur solve's history, relative to |b_e + k D_eo b_o|) and
// `k = ...: converged / did not converge after N steps, |x|^2 = ...` for the reconstructed full solution.
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
    if (ks.empty()) {
        std::fprintf(stderr, "usage: %s [matrix file] k_1 [k_2 ...]   (k_j: re or re,im)\n", argv[0]);
        return 2;
    }
    long dims[6] = {4, 4, 4, 4, 4, 3};
    auto D = new Sparse(read_data(file));
    if (D->get_dim() != 3072) { dims[0] = dims[1] = dims[2] = dims[3] = 8; }   // the 8x8 configuration's mesh

    Field<long> rhs(dims, 6);
    rhs.init_rand(0);
    GCR_Param<long> param(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    EvenOddDiracOp<long> eo(D, ks[0]);           // the rows are two-coloured once; the ladder only changes k
    std::printf("even-odd: %ld rows, %ld even, %ld odd\n", eo.get_n(), eo.get_n_even(), eo.get_n_odd());
    for (size_t j = 0; j < ks.size(); j++) {
        eo.set_k(ks[j]);
        Field<long> sol(rhs.get_mesh());
        sol.set_zero();
        eo.solve(rhs, sol, &param);
        for (int i = 0; i <= eo.last_iterations; i++) std::printf("[%d] Step %d residual norm = %.10e\n", (int)j, i, eo.last_history[(size_t)i]);
        char name[64];
        if (ks[j].imag() != 0.) std::snprintf(name, sizeof name, "%g%+gi", ks[j].real(), ks[j].imag());
        else std::snprintf(name, sizeof name, "%g", ks[j].real());
        std::printf("k = %s: %s after %d steps, |x|^2 = %.10e\n", name, eo.last_converged ? "converged" : "did not converge", eo.last_iterations,
                    sol.squarednorm());
    }
    delete D;
    return 0;
}
