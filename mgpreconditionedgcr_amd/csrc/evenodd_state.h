// The state of an even-odd preconditioned DiracOp (OP_DIRAC_EO), shared by evenodd.hip, which makes and owns it, and
// evenodd_multi.hip, whose operators borrow its two half matrices and index lists.
#pragma once
#include <vector>

#include "internal.h"

namespace mgcr {

struct EvenOddPlan;   // evenodd_plan.h

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
    // The site diagonal (evenodd_diag.hip, mgcr_eo_create_diag): A = diag(a) - c H with H the two halves.  Dirac form: a = 1 - k d,
    // c = k; matrix form: a = d, c = -1.  has_diag false: everything below is unused and every call takes evenodd.hip's own path.
    bool has_diag = false, matrix_form = false;
    std::vector<cplx> h_d_even, h_d_odd;               // d in list order, on the host (the singular check of set_k)
    cplx *dd_even = nullptr, *dd_odd = nullptr;        // ... and on the device
    cplx *a_even = nullptr, *inv_a_odd = nullptr;      // [n_e] a, [n_o] 1 / a: written in stream order by diag_coeff_kernel
    cplx c = {0., 0.}, c2 = {0., 0.}, cn = {0., 0.};   // c, c c and -c, formed once on the host
    // The site blocks (evenodd_block.hip, mgcr_eo_create_block): A = B - c H, B one dense bs x bs block per site of bs consecutive rows,
    // H the entries between different sites.  Dirac form: B_s = I - k D_ss, c = k; matrix form: B_s = D_ss, c = -1 (matrix_form, c, c2
    // and cn above are shared with the site diagonal; has_diag stays false).  has_block false: everything below is unused.
    bool has_block = false;
    int32_t bs = 0;
    int64_t sites_e = 0, sites_o = 0;
    cplx *dblk_even = nullptr, *dblk_odd = nullptr;    // [sites][bs][bs] D_ss as stored, in list order
    cplx *B_even = nullptr, *invB_odd = nullptr;       // B of the even sites, B^-1 of the odd ones: what the applies read (block column
                                                       // outermost: entry (r, c) of half-site s at [c * n_half + s * bs + r])
    cplx *invB_spare = nullptr;                        // where blk_invert_kernel works: swapped with invB_odd once the host has seen it succeed
    unsigned long long *blk_status = nullptr;          // the status word of blk_invert_kernel (one per operator)
};

// k k as mgcr_eo_set_k forms it: on the host, un-fused
inline cplx host_cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// ---- evenodd.hip's host pieces that evenodd_diag.hip builds on ---------------------------------------------------------------
int eo_split(const EoState *e, const cplx *full, cplx *even, cplx *odd);
int eo_merge(const EoState *e, cplx *full, const cplx *even, const cplx *odd);
int eo_work(EoState *e, EoState::Work which, cplx **out);
int eo_shift_apply(EoState *e, int h, const cplx *x, cplx *y, cplx c, const cplx *w);   // y = w - c (H x), bits of "u = H x; y = w - c u"
int eo_build_halves(EoState *e, const EvenOddPlan &plan, const char *who);   // the two Sparse halves, the index lists and t

// ---- evenodd_diag.hip: the same four operations on an operator with a site diagonal (EoState::has_diag) ------------------------
void eo_diag_destroy(EoState *e);
int eo_diag_set_k(Op *op, cplx k);
int eo_diag_apply(EoState *e, const cplx *x, cplx *y);
bool eo_diag_schur_fusable(const EoState *e);
int eo_diag_schur_step(EoState *e, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm);
int eo_diag_prepare(EoState *e, const cplx *b_full, cplx *bhat);
int eo_diag_reconstruct(EoState *e, const cplx *b_full, const cplx *xe, cplx *x_full);

// ---- evenodd_block.hip: ... and on an operator with a dense block per site (EoState::has_block) ---------------------------------
void eo_block_destroy(EoState *e);
int eo_block_set_k(Op *op, cplx k);
int eo_block_apply(EoState *e, const cplx *x, cplx *y);
bool eo_block_schur_fusable(const EoState *e);
int eo_block_schur_step(EoState *e, const cplx *x, cplx *y, const cplx *const *vecs, int nd, double *parts, const RowMap &rm);
int eo_block_prepare(EoState *e, const cplx *b_full, cplx *bhat);
int eo_block_reconstruct(EoState *e, const cplx *b_full, const cplx *xe, cplx *x_full);

}  // namespace mgcr
