// A hopping-parameter scan as ONE batched solve: (1 - k_j D) x_j = b for a list of k_j, the same D and the same right-hand
// side in every column — what test_kcritical (src/main.cpp:696-741) does with one DiracOp and one solve per value.  The
// k_j are the shifts per column of a MultiDiracOp; D is streamed once per step for all of them, a column that has
// converged is frozen while the others go on.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/k_critical_batched [matrix file] k_1 [k_2 ...]
//
// k_j: `re` or `re,im`; at most 16 of them.  GCR(5), at most 400 steps, tolerance 1e-10, rhs init_rand(0), x0 = 0.
// Prints, per column, `[j] Step i residual norm = ...` and `k = ...: converged / did not converge after N steps`.
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
        if (end == argv[a] || (*end != '\0' && !(*end == ',' && end2 != end + 1 && *end2 == '\0'))) {   // not `re` or `re,im`: the matrix file
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
    auto Dirac = new MultiDiracOp<long>(D, ks);

    Field<long> rhs(dims, 6);
    rhs.init_rand(0);
    const int k = (int)ks.size();
    MultiField<long> B(std::vector<const Field<long> *>((size_t)k, &rhs));
    MultiField<long> X(rhs.get_mesh(), k);
    X.set_zero();

    GCR_Param<long> param(0, 5, 400, 1e-10, false, nullptr, nullptr);
    GCR gcr(Dirac, &param);
    gcr.solve_multi(B, X);                       // ONE solve for the whole ladder

    for (int j = 0; j < k; j++)
        for (int i = 0; i <= gcr.last_iterations[(size_t)j]; i++)
            std::printf("[%d] Step %d residual norm = %.10e\n", j, i, gcr.last_history[(size_t)j][(size_t)i]);
    for (int j = 0; j < k; j++) {
        const std::complex<double> kj = ks[(size_t)j];
        char name[64];
        if (kj.imag() != 0.) std::snprintf(name, sizeof name, "%g%+gi", kj.real(), kj.imag());
        else std::snprintf(name, sizeof name, "%g", kj.real());
        std::printf("k = %s: %s after %d steps\n", name, gcr.last_converged[(size_t)j] ? "converged" : "did not converge", gcr.last_iterations[(size_t)j]);
    }
    delete Dirac;
    delete D;
    return 0;
}
