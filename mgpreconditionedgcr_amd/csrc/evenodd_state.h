// The state of an even-odd preconditioned DiracOp (OP_DIRAC_EO), shared by evenodd.hip, which makes and owns it, and
// evenodd_multi.hip, whose operators borrow its two half matrices and index lists.
#pragma once
#include <vector>

#include "internal.h"

namespace mgcr {

struct EoState {
    int64_t n = 0, ne = 0, no = 0, nnz = 0;
    std::vector<int8_t> parity;
    int32_t *d_even = nullptr, *d_odd = nullptr;   // the index lists
    mgcr_op_s *half[2] = {nullptr, nullptr};       // D_eo (n_e x n_o), D_oe (n_o x n_e): Sparse operators, owned (mgcr_eo_half_op lends them)
    cplx k = {0., 0.}, k2 = {0., 0.};
    cplx *t = nullptr;                             // [n_o] D_oe x between the two stages
    // work Fields, allocated on first use (eo_work).  W_BE, W_BO: the halves of b (prepare; reconstruct rewrites W_BO); W_BHAT, W_XE:
    // right-hand side and iterate of mgcr_eo_solve's Schur solve; W_XO: the odd half before the merge; W_UE, W_UO: the product of a
    // half with a CSR tail before it is subtracted (eo_shift_apply).  W_BO, W_XO and W_UO have n_o entries, the others n_e.
    enum Work { W_BE, W_BO, W_BHAT, W_XE, W_XO, W_UE, W_UO, W_COUNT };
    cplx *work[W_COUNT] = {};
    // the solver of mgcr_eo_solve: kept between calls with its Krylov vectors, like a GCR object's (a k ladder allocates once)
    GcrState *solver = nullptr;
};

// k k as mgcr_eo_set_k forms it: on the host, un-fused
inline cplx host_cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

}  // namespace mgcr
