// An even-odd hopping-parameter scan through a QUEUE: (1 - k_j D) x_j = b for any number of k_j, every system solved as its Schur
// system on the even half of the lattice and streamed through `width` columns of one batched solve — a column whose k has stopped
// is reconstructed and takes the next waiting k at the next boundary of the restart cycle (EvenOddDiracOp::solve_queue).
// examples/k_critical_evenodd_batched.cpp is the form with one column per k (at most 16, all waiting for the slowest),
// examples/k_critical_queue.cpp the queue on the full systems.
//
//   make -C examples
//   MGCR_SAMPLE_DIR=<dir with 4x4parsed.txt> examples/build/k_critical_evenodd_queue [matrix file] width k_1 [k_2 ...]
//
// k_j: `re` or `re,im`.  GCR(5), at most 4000 steps, tolerance 1e-10, rhs init_rand(0), x0 = 0.
// Prints the lines of k_critical_evenodd_batched: per k, `[j] Step i residual norm = ...` (the Schur solve's history, relative to
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
    int width = 0;
    for (int a = 1; a < argc; a++) {
        char *end = nullptr, *end2 = nullptr;
        const double re = std::strtod(argv[a], &end);
        const double im = end != argv[a] && *end == ',' ? std::strtod(end + 1, &end2) : 0.;
        if (end == argv[a] || (*end != '\0' && !(*end == ',' && end2 != end + 1 && *end2 == '\0'))) {   // not a number: the matrix file
            file = argv[a];
            continue;
        }
        if (width == 0) width = (int)re;
        else ks.push_back(std::complex<double>(re, im));
    }
    if (ks.empty() || width < 1 || width > 16) {
        std::fprintf(stderr, "usage: %s [matrix file] width k_1 [k_2 ...]   (width: 1 .. 16; k_j: re or re,im)\n", argv[0]);
        return 2;
    }
    long dims[6] = {4, 4, 4, 4, 4, 3};
    auto D = new Sparse(read_data(file));
    if (D->get_dim() != 3072) { dims[0] = dims[1] = dims[2] = dims[3] = 8; }   // the 8x8 configuration's mesh

    Field<long> rhs(dims, 6);
    rhs.init_rand(0);
    const size_t n = ks.size();
    std::vector<Field<long>> sol(n, Field<long>(rhs.get_mesh()));
    std::vector<const Field<long> *> b(n, &rhs);
    std::vector<Field<long> *> x;
    for (Field<long> &f : sol) { f.set_zero(); x.push_back(&f); }

    GCR_Param<long> param(0, 5, 4000, 1e-10, false, nullptr, nullptr);
    {
        EvenOddDiracOp<long> eo(D, ks[0]);           // the rows are two-coloured once; its own k is not used below
        std::printf("even-odd: %ld rows, %ld even, %ld odd\n", eo.get_n(), eo.get_n_even(), eo.get_n_odd());
        eo.solve_queue(b, x, ks, &param, width);     // ONE call for the whole ladder, however long

        for (size_t j = 0; j < n; j++)
            for (int i = 0; i <= eo.queue_iterations[j]; i++) std::printf("[%d] Step %d residual norm = %.10e\n", (int)j, i, eo.queue_history[j][(size_t)i]);
        for (size_t j = 0; j < n; j++) {
            char name[64];
            if (ks[j].imag() != 0.) std::snprintf(name, sizeof name, "%g%+gi", ks[j].real(), ks[j].imag());
            else std::snprintf(name, sizeof name, "%g", ks[j].real());
            std::printf("k = %s: %s after %d steps, |x|^2 = %.10e\n", name, eo.queue_converged[j] ? "converged" : "did not converge", eo.queue_iterations[j],
                        sol[j].squarednorm());
        }
    }
    delete D;
    return 0;
}
