// The state of a MultiEvenOddDiracOp (OP_DIRAC_EO_MULTI) and the k-wide shifted half applies, shared by evenodd_multi.hip, which
// makes the operator, and evenodd_queue.hip, whose slot operator is one.
#pragma once
#include "internal.h"
#include "multi_dev.h"
#include "evenodd_state.h"

namespace mgcr {

struct EoMultiState {
    Op *eo = nullptr;   // the OP_DIRAC_EO whose halves and lists are read (borrowed: it outlives this operator)
    KCols ks2;          // k_j k_j (the k_j themselves are Op::ks); entries from nk on are 0 and are not read
    cplx *t = nullptr;  // [n_o x nk] D_oe X between the two stages, allocated on first use
    // work blocks, allocated on first use, the roles of EoState::Work: W_BO, W_XO and W_UO have n_o rows, the others n_e
    cplx *work[EoState::W_COUNT] = {};
};

// the operator's work block `which` (EoState::Work), allocated on first use
int eom_work(Op *op, EoState::Work which, cplx **out);
// Y_j = W_j - c_j (H X)_j for half H (0: D_eo, 1: D_oe), every column; a half with a CSR tail goes through W_UE / W_UO
int eom_shift_apply(Op *op, int h, const cplx *x, cplx *y, const KCols &cs, const cplx *w);
// the factors -k_j of prepare and reconstruct
KCols eom_negated(const Op *op);

}  // namespace mgcr
