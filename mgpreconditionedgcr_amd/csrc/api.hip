// Operator / solver part of the C ABI (include/mgcr.h).
#include <algorithm>
#include <numeric>

#include <cstring>

#include "internal.h"

using namespace mgcr;

#define LOCK() std::lock_guard<std::recursive_mutex> lk__(ctx().mtx)

extern "C" {

int mgcr_csr_create(int64_t nrow, int64_t ncol, const int64_t *rowptr, const int64_t *col, const double *val_ri,
                    mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && rowptr && (col || rowptr[nrow] == 0) && (val_ri || rowptr[nrow] == 0), MGCR_ERR_INVALID,
               "mgcr_csr_create: null argument");
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_CSR;
    op->dim = ncol;
    op->nrow = nrow;
    int rc = csr_build_device(nrow, ncol, rowptr, col, val_ri, &op->csr);
    if (rc != MGCR_OK) { delete op; return rc; }
    *out = op;
    return MGCR_OK;
}

int mgcr_csr_replace(mgcr_op_t op, int64_t nrow, int64_t ncol, const int64_t *rowptr, const int64_t *col, const double *val_ri) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(op && rowptr && (col || rowptr[nrow] == 0) && (val_ri || rowptr[nrow] == 0), MGCR_ERR_INVALID, "mgcr_csr_replace: null argument");
    MGCR_CHECK(op->kind == OP_CSR && !op->dist, MGCR_ERR_INVALID, "mgcr_csr_replace: not a (single-GPU) Sparse");
    LOCK();
    MGCR_HIP(hipStreamSynchronize(ctx().stream));   // nothing queued may still read the old matrix
    CsrDev fresh;
    MGCR_TRY(csr_build_device(nrow, ncol, rowptr, col, val_ri, &fresh));
    csr_free(&op->csr);
    op->csr = fresh;
    op->dim = ncol;
    op->nrow = nrow;
    return MGCR_OK;
}

int mgcr_dirac_create(mgcr_op_t csr, const double k_ri[2], mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(csr && k_ri && out, MGCR_ERR_INVALID, "mgcr_dirac_create: null argument");
    MGCR_CHECK(csr->kind == OP_CSR, MGCR_ERR_INVALID, "mgcr_dirac_create: DiracOp wraps a Sparse (CSR) operator");
    // (the row block of a distributed Sparse has its halo columns appended: square means dim == nrow there)
    MGCR_CHECK(csr->dist ? csr->dim == csr->nrow : csr->csr.nrow == csr->csr.ncol, MGCR_ERR_INVALID, "mgcr_dirac_create: matrix must be square");
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC;
    op->dim = csr->dim;
    op->nrow = csr->nrow;
    op->comm = csr->comm;
    op->base = csr;
    op->k = make_double2(k_ri[0], k_ri[1]);
    *out = op;
    return MGCR_OK;
}

int mgcr_dirac_set_k(mgcr_op_t dirac, const double k_ri[2]) {
    MGCR_CHECK(dirac && k_ri && dirac->kind == OP_DIRAC, MGCR_ERR_INVALID, "mgcr_dirac_set_k: not a DiracOp");
    LOCK();
    dirac->k = make_double2(k_ri[0], k_ri[1]);
    return MGCR_OK;
}

static int dirac_multi_values(const double *k_ri, int32_t k, cplx *out, const char *who) {
    for (int32_t j = 0; j < k; j++) {
        MGCR_CHECK(k_ri[2 * j] != 0. || k_ri[2 * j + 1] != 0., MGCR_ERR_INVALID, "%s: k[%d] is zero (No k value supplied for Dirac Operator!)", who, (int)j);
        out[j] = make_double2(k_ri[2 * j], k_ri[2 * j + 1]);
    }
    return MGCR_OK;
}

int mgcr_dirac_multi_create(mgcr_op_t csr, int32_t k, const double *k_ri, mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(csr && k_ri && out, MGCR_ERR_INVALID, "mgcr_dirac_multi_create: null argument");
    MGCR_CHECK(csr->kind == OP_CSR, MGCR_ERR_INVALID, "mgcr_dirac_multi_create: MultiDiracOp wraps a Sparse (CSR) operator");
    MGCR_CHECK(!csr->dist && !csr->comm, MGCR_ERR_UNSUPPORTED, "mgcr_dirac_multi_create: distributed operators are not supported");
    MGCR_CHECK(csr->csr.nrow == csr->csr.ncol, MGCR_ERR_INVALID, "mgcr_dirac_multi_create: matrix must be square");
    MGCR_CHECK(k >= 1 && k <= MV_MAX_K, MGCR_ERR_INVALID, "mgcr_dirac_multi_create: k = %d hopping parameters, 1 .. %d are supported", (int)k, MV_MAX_K);
    cplx ks[MV_MAX_K] = {};
    MGCR_TRY(dirac_multi_values(k_ri, k, ks, "mgcr_dirac_multi_create"));
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_DIRAC_MULTI;
    op->dim = csr->dim;
    op->nrow = csr->nrow;
    op->base = csr;
    op->nk = k;
    std::copy(ks, ks + MV_MAX_K, op->ks);
    *out = op;
    return MGCR_OK;
}

// The values travel in the kernel arguments of every launch (KCols, multi_dev.h): what is already enqueued keeps the old ones.
int mgcr_dirac_multi_set_k(mgcr_op_t op, const double *k_ri) {
    MGCR_CHECK(op && k_ri && op->kind == OP_DIRAC_MULTI, MGCR_ERR_INVALID, "mgcr_dirac_multi_set_k: not a MultiDiracOp");
    cplx ks[MV_MAX_K] = {};
    MGCR_TRY(dirac_multi_values(k_ri, op->nk, ks, "mgcr_dirac_multi_set_k"));
    LOCK();
    std::copy(ks, ks + MV_MAX_K, op->ks);
    return MGCR_OK;
}

int mgcr_bcsr_create(int32_t nbrow, int32_t nbcol, int32_t bs, const int32_t *browptr, const int32_t *bcol,
                     const double *blocks_ri, mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(out && browptr && bcol && blocks_ri, MGCR_ERR_INVALID, "mgcr_bcsr_create: null argument");
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_BCSR;
    int rc = bcsr_build_device(nbrow, nbcol, bs, browptr, bcol, blocks_ri, &op->bcsr);
    if (rc != MGCR_OK) { delete op; return rc; }
    op->dim = (int64_t)nbcol * bs;  // this->dim = block_cols * sub_dim, src/HierarchicalSparse.h:62
    op->nrow = (int64_t)nbrow * bs;
    *out = op;
    return MGCR_OK;
}

// HierarchicalSparse constructor (src/HierarchicalSparse.h:58-98): sort the triplets by
// row*nbcol+col, keep duplicates.  Unlike the reference we accept empty block-rows and a first
// triplet outside row 0 (its row counter would mis-assign those), and the sort is
// stable.
int mgcr_bcsr_create_from_triplets(int32_t nbrow, int32_t nbcol, int32_t bs, int32_t ntriplets, const int32_t *rows,
                                   const int32_t *cols, const double *blocks_ri, mgcr_op_t *out) {
    MGCR_CHECK(out && rows && cols && blocks_ri && ntriplets >= 0, MGCR_ERR_INVALID,
               "mgcr_bcsr_create_from_triplets: bad argument");
    for (int32_t t = 0; t < ntriplets; t++)
        MGCR_CHECK(rows[t] >= 0 && rows[t] < nbrow && cols[t] >= 0 && cols[t] < nbcol, MGCR_ERR_INVALID,
                   "triplet %d: block index (%d,%d) out of range", t, rows[t], cols[t]);
    std::vector<int32_t> order((size_t)ntriplets);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return (int64_t)rows[a] * nbcol + cols[a] < (int64_t)rows[b] * nbcol + cols[b];
    });
    std::vector<int32_t> browptr((size_t)nbrow + 1, 0), bcol((size_t)ntriplets);
    std::vector<double> blocks((size_t)ntriplets * bs * bs * 2);
    const size_t bsz = (size_t)bs * bs * 2;
    for (int32_t t = 0; t < ntriplets; t++) {
        int32_t s = order[(size_t)t];
        bcol[(size_t)t] = cols[s];
        std::copy(blocks_ri + (size_t)s * bsz, blocks_ri + (size_t)(s + 1) * bsz, blocks.begin() + (size_t)t * bsz);
        browptr[(size_t)rows[s] + 1]++;
    }
    for (int32_t r = 0; r < nbrow; r++) browptr[(size_t)r + 1] += browptr[(size_t)r];
    return mgcr_bcsr_create(nbrow, nbcol, bs, browptr.data(), bcol.data(), blocks.data(), out);
}

int mgcr_op_destroy(mgcr_op_t op) {
    if (!op) return MGCR_OK;
    LOCK();
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    switch (op->kind) {
        case OP_CSR: csr_free(&op->csr); dist_free(op->dist); break;
        case OP_BCSR: bcsr_free(&op->bcsr); dist_free(op->dist); break;
        case OP_GCR: gcr_state_destroy(op->gcr); break;
        case OP_MG: mg_destroy(op->mg); break;
        case OP_DIRAC_EO: eo_destroy(op->eo); break;
        case OP_GCR32: gcr32_destroy(op->g32); break;
        case OP_DIRAC_EO_MULTI: eo_multi_destroy(op->eom); break;   // (the even-odd operator behind it is borrowed)
        default: break;  // OP_DIRAC and OP_DIRAC_MULTI borrow their Sparse (src/Operator.h:117,555-560)
    }
    delete op;
    return MGCR_OK;
}

int64_t mgcr_op_dim(mgcr_op_t op) { return op ? op->dim : -1; }
int64_t mgcr_op_nrow(mgcr_op_t op) { return op ? op->nrow : -1; }
int64_t mgcr_op_nnz(mgcr_op_t op) {
    if (!op) return -1;
    switch (op->kind) {
        case OP_CSR: return op->csr.nnz;
        case OP_DIRAC:
        case OP_DIRAC_MULTI: return op->base->csr.nnz;
        case OP_BCSR: return (int64_t)op->bcsr.nblocks * op->bcsr.bs * op->bcsr.bs;  // src/HierarchicalSparse.h:31
        case OP_DIRAC_EO: return eo_nnz(op->eo);   // that of D
        case OP_DIRAC_EO_MULTI: return eo_multi_nnz(op->eom);
        case OP_GCR32: return gcr32_nnz(op->g32);   // that of the matrix it copied
        default: return -1;
    }
}

int mgcr_op_storage_format(mgcr_op_t op, int32_t *format, int32_t *n_patterns) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_storage_format");
    MGCR_REFUSE_GCR32(op, "mgcr_op_storage_format");
    const Op *o = op_matrix(op);
    MGCR_CHECK(o->kind == OP_CSR, MGCR_ERR_UNSUPPORTED, "mgcr_op_storage_format: not a Sparse");
    if (format) *format = csr_stencil_active(o->csr) ? 3 : o->csr.pat_mode;
    if (n_patterns) *n_patterns = csr_stencil_active(o->csr) ? o->csr.sten_ns : o->csr.npat;
    return MGCR_OK;
}

int mgcr_op_ell_layout(mgcr_op_t op, int32_t *ell_width, int32_t *lanes, int64_t *tail_rows, int64_t *reach, int32_t *tail_chunk_cap,
                       int32_t *x_window) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_ell_layout");
    MGCR_REFUSE_GCR32(op, "mgcr_op_ell_layout");
    const Op *o = op_matrix(op);
    MGCR_CHECK(o->kind == OP_CSR, MGCR_ERR_UNSUPPORTED, "mgcr_op_ell_layout: not a Sparse");
    if (ell_width) *ell_width = o->csr.W;
    if (lanes) *lanes = o->csr.L;
    if (tail_rows) *tail_rows = o->csr.n_tail_rows;
    if (reach) *reach = o->csr.reach;
    if (tail_chunk_cap) *tail_chunk_cap = TAIL_CAP;
    if (x_window) *x_window = o->csr.win_h;
    return MGCR_OK;
}

int mgcr_op_xr_fuse_kind(mgcr_op_t op, int32_t *kind) {
    MGCR_CHECK(op && kind, MGCR_ERR_INVALID, "mgcr_op_xr_fuse_kind: null argument");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_xr_fuse_kind");
    MGCR_REFUSE_GCR32(op, "mgcr_op_xr_fuse_kind");
    const Op *o = op_matrix(op);
    MGCR_CHECK(o->kind == OP_CSR, MGCR_ERR_UNSUPPORTED, "mgcr_op_xr_fuse_kind: not a Sparse");
    *kind = csr_fusable(o->csr, o->dist) ? csr_xr_fuse_kind(o->csr, o->dist) : 0;
    return MGCR_OK;
}

int mgcr_op_halo_kind(mgcr_op_t op, int32_t *kind) {
    MGCR_CHECK(op && kind, MGCR_ERR_INVALID, "mgcr_op_halo_kind: null argument");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_halo_kind");
    MGCR_REFUSE_GCR32(op, "mgcr_op_halo_kind");
    const Op *o = op_matrix(op);
    MGCR_CHECK(o->dist, MGCR_ERR_UNSUPPORTED, "mgcr_op_halo_kind: not a distributed Sparse");
    *kind = dist_halo_kind(o->dist);
    return MGCR_OK;
}

int mgcr_set_option(const char *name, int value, int *previous) {
    MGCR_CHECK(name, MGCR_ERR_INVALID, "null option name");
    if (!strcmp(name, "spmv_part")) {   // measurement aid: 0 whole apply, 1 ELL slab only, 2 CSR tail only (spmv.hip)
        const int p = set_spmv_part(value);
        if (previous) *previous = p;
        return MGCR_OK;
    }
    if (!strcmp(name, "step_build_pair_late")) {   // 0 off, 1 the late-r pair forms that cleared their gate, 2 every built one (gcr_steppair_late.hip)
        const int p = set_stepbuild_pair_late(value);
        if (previous) *previous = p;
        return MGCR_OK;
    }
    bool prev;
    if (!strcmp(name, "pattern_storage")) prev = set_patterns_enabled(value != 0);
    else if (!strcmp(name, "stencil_storage")) prev = set_stencil_enabled(value != 0);
    else if (!strcmp(name, "lean_cycles")) prev = set_lean_enabled(value != 0);
    else if (!strcmp(name, "fused_apply")) prev = set_fuse_enabled(value != 0);
    else if (!strcmp(name, "graph_replay")) prev = set_graph_enabled(value != 0);
    else if (!strcmp(name, "resident_solver")) prev = set_resident_enabled(value != 0);
    else if (!strcmp(name, "step_build")) prev = set_stepbuild_enabled(value != 0);
    else if (!strcmp(name, "start_build")) prev = set_start_build_enabled(value != 0);
    else if (!strcmp(name, "step_build_keep_r")) {   // accepted, without effect: step_keep_kernel took over those steps
        static bool last = true;
        prev = last;
        last = value != 0;
    }
    else if (!strcmp(name, "step_build_keep_all")) prev = set_stepbuild_keep_all_enabled(value != 0);
    else if (!strcmp(name, "step_build_pair")) prev = set_stepbuild_pair_enabled(value != 0);
    else if (!strcmp(name, "halo_split")) prev = set_halo_split(value != 0);
    else if (!strcmp(name, "pw_tail")) prev = set_pw_tail_enabled(value != 0);
    else { set_error("mgcr_set_option: unknown option '%s'", name); return MGCR_ERR_INVALID; }
    if (previous) *previous = prev ? 1 : 0;
    return MGCR_OK;
}

int mgcr_stat(const char *name, int64_t *value) {
    MGCR_CHECK(name && value, MGCR_ERR_INVALID, "mgcr_stat: null argument");
    if (!strcmp(name, "resident_solves")) *value = resident_solve_count();
    // The three step counters count steps by FORM, not by kernel symbol: every one-launch step | those at >= 4 directions that read
    // r once | those whose apply takes its own r from the diagonal gather.  A step that runs as step_pair_kernel (gcr_steppair.hip)
    // or step_pair_late_kernel (gcr_steppair_late.hip) is counted by each of them it belongs to; step_pair_launches (a pair kernel
    // at 1..4 directions) and step_pair_late_launches (the late-r kernel, the close at 5 included) say which kernel ran.
    else if (!strcmp(name, "step_build_launches")) *value = stepbuild_launch_count();
    else if (!strcmp(name, "step_keep_wide_launches")) *value = stepbuild_keep_wide_launch_count();
    else if (!strcmp(name, "step_apply_own_launches")) *value = stepbuild_apply_own_launch_count();
    else if (!strcmp(name, "step_pair_launches")) *value = stepbuild_pair_launch_count();
    else if (!strcmp(name, "step_pair_late_launches")) *value = stepbuild_pair_late_launch_count();
    else if (!strcmp(name, "start_build_launches")) *value = start_build_launch_count();
    else if (!strcmp(name, "small_solves")) *value = gcr_small_solve_count();
    else if (!strcmp(name, "one_launch_fallbacks")) *value = gcr_fallback_count();
    else if (!strcmp(name, "halo_split_exchanges")) *value = dist_halo_split_count();
    else if (!strcmp(name, "pw_tail_folds")) *value = comm_pw_tail_count();
    else if (!strcmp(name, "multi_solves")) *value = gcr_multi_solve_count();
    else if (!strcmp(name, "multi_flex_solves")) *value = gcr_multi_flex_solve_count();
    else if (!strcmp(name, "queue_solves")) *value = gcr_queue_stat(0);
    else if (!strcmp(name, "queue_admissions")) *value = gcr_queue_stat(1);
    else if (!strcmp(name, "queue_steps")) *value = gcr_queue_stat(2);
    else if (!strcmp(name, "eo_queue_solves")) *value = gcr_queue_stat(3);
    else if (!strcmp(name, "eo_queue_admissions")) *value = gcr_queue_stat(4);
    else if (!strcmp(name, "eo_queue_steps")) *value = gcr_queue_stat(5);
    else if (!strcmp(name, "evenodd_fused_steps")) *value = eo_fused_step_count();
    else if (!strcmp(name, "evenodd_diag_fused_steps")) *value = eo_diag_fused_step_count();
    else if (!strcmp(name, "evenodd_block_applies")) *value = eo_block_apply_count();
    else if (!strcmp(name, "evenodd_block_fused_steps")) *value = eo_block_fused_step_count();
    else if (!strcmp(name, "gcr32_applies")) *value = gcr32_apply_count();
    else if (!strcmp(name, "gcr32_steps")) *value = gcr32_step_count();
    else if (!strcmp(name, "gcr32_multi_applies")) *value = gcr32_multi_stat(0);
    else if (!strcmp(name, "gcr32_multi_steps")) *value = gcr32_multi_stat(1);
    else { set_error("mgcr_stat: unknown counter '%s'", name); return MGCR_ERR_INVALID; }
    return MGCR_OK;
}

int mgcr_selftest_coherence(int32_t steps, int32_t coherent, int64_t *rows_wrong) {
    MGCR_TRY(require_ctx());
    LOCK();
    return coherence_selftest(steps, coherent, rows_wrong);
}

int mgcr_op_stored_bytes(mgcr_op_t op, int64_t *matrix_bytes, int32_t *ell_width, int64_t *tail_nnz) {
    MGCR_CHECK(op, MGCR_ERR_INVALID, "null operator");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_stored_bytes");
    MGCR_REFUSE_GCR32(op, "mgcr_op_stored_bytes");
    const Op *o = op_matrix(op);
    if (o->kind == OP_CSR) {
        const CsrDev &A = o->csr;
        int64_t slab = (int64_t)A.nchunk * A.npad * A.L;
        int64_t ell_bytes = slab * (A.ell_val_re ? 12 : 20);
        if (csr_stencil_active(A)) ell_bytes = (A.npad / 64) * A.sten_stride * 8 + A.sten_kernel_ns * 20;   // presence words + slot table
        else if (A.pat_mode == 1) ell_bytes = A.npad * 2 + (int64_t)A.npat * A.W * (A.pat_real ? 12 : 20);
        else if (A.pat_mode == 2) ell_bytes = A.npad * 2 + (int64_t)A.npat * A.W * 4 + slab * (A.ell_val_re ? 8 : 16);
        if (matrix_bytes) *matrix_bytes = ell_bytes + A.tail_nnz * 20 + A.n_tail_rows * 8 + (A.n_tail_rows ? 4 : 0);
        if (ell_width) *ell_width = A.nchunk * A.L;
        if (tail_nnz) *tail_nnz = A.tail_nnz;
        return MGCR_OK;
    }
    if (o->kind == OP_BCSR) {
        const BcsrDev &B = o->bcsr;
        if (matrix_bytes) *matrix_bytes = (int64_t)B.nblocks * (16LL * B.bs * B.bs + 4) + ((int64_t)B.nbrow + 1) * 4;
        if (ell_width) *ell_width = 0;
        if (tail_nnz) *tail_nnz = 0;
        return MGCR_OK;
    }
    set_error("mgcr_op_stored_bytes: not a matrix operator");
    return MGCR_ERR_UNSUPPORTED;
}

int mgcr_op_apply(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(op && x && y, MGCR_ERR_INVALID, "mgcr_op_apply: null argument");
    MGCR_REFUSE_MULTI_DIRAC(op, "mgcr_op_apply");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_op_apply");
    MGCR_CHECK(x->n == op->dim, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
    int64_t nrow = op->nrow ? op->nrow : op->dim;
    MGCR_CHECK(y->n == nrow, MGCR_ERR_INVALID, "output Field has %lld entries, operator has %lld rows", (long long)y->n, (long long)nrow);
    // no operator applies in place: the matrix kernels gather from x while they write y, and an MG / GCR operator reads its
    // input again after it has started to write the output (post-smoother, x0 handling)
    MGCR_CHECK(x->d != y->d, MGCR_ERR_INVALID, "mgcr_op_apply: input and output must be different Fields");
    LOCK();
    return op_apply_raw(op, x->d, y->w(), x->n);
}

int mgcr_gcr_solve(mgcr_op_t A, const mgcr_gcr_param *param, mgcr_vec_t rhs, mgcr_vec_t x, double *hist, int32_t hist_cap,
                   int32_t *n_iter, int32_t *converged) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(A && param && rhs && x, MGCR_ERR_INVALID, "mgcr_gcr_solve: null argument");
    MGCR_REFUSE_MULTI_DIRAC(A, "mgcr_gcr_solve");
    MGCR_REFUSE_EVENODD_MULTI(A, "mgcr_gcr_solve");
    MGCR_REFUSE_GCR32(A, "mgcr_gcr_solve");
    // assertm(rhs.field_size() == this->dim, ...) src/GCR.h:160-161
    MGCR_CHECK(rhs->n == A->dim, MGCR_ERR_INVALID, "Field dimension does not match with Operator!");
    MGCR_CHECK(x->n == A->dim, MGCR_ERR_INVALID, "x dimension does not match with Operator!");
    MGCR_CHECK(rhs->d != x->d, MGCR_ERR_INVALID, "rhs and x must be different Fields");
    LOCK();
    GcrState *s = nullptr;
    MGCR_TRY(gcr_state_create(A, param, 1, &s));
    int it = 0, conv = 0;
    const bool xz = x->zero_known;
    int rc = gcr_run(s, rhs->d, x->w(), false, hist, hist_cap, &it, &conv, xz);
    gcr_state_destroy(s);
    if (n_iter) *n_iter = it;
    if (converged) *converged = conv;
    return rc;
}

int mgcr_gcr_create(mgcr_op_t A, const mgcr_gcr_param *param, int32_t x0_mode, mgcr_op_t *out) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(param && out, MGCR_ERR_INVALID, "mgcr_gcr_create: null argument");
    MGCR_REFUSE_MULTI_DIRAC(A, "mgcr_gcr_create");
    MGCR_REFUSE_EVENODD_MULTI(A, "mgcr_gcr_create");
    MGCR_REFUSE_GCR32(A, "mgcr_gcr_create");
    LOCK();
    mgcr_op_s *op = new mgcr_op_s();
    op->kind = OP_GCR;
    op->dim = A ? A->dim : 0;
    op->nrow = op->dim;
    int rc = gcr_state_create(A, param, x0_mode, &op->gcr);
    if (rc != MGCR_OK) { delete op; return rc; }
    *out = op;
    return MGCR_OK;
}

int mgcr_gcr_set_operator(mgcr_op_t gcr, mgcr_op_t A) {
    MGCR_CHECK(gcr && A && gcr->kind == OP_GCR, MGCR_ERR_INVALID, "mgcr_gcr_set_operator: not a GCR operator");
    MGCR_REFUSE_MULTI_DIRAC(A, "mgcr_gcr_set_operator");
    MGCR_REFUSE_EVENODD_MULTI(A, "mgcr_gcr_set_operator");
    MGCR_REFUSE_GCR32(A, "mgcr_gcr_set_operator");
    LOCK();
    gcr->dim = A->dim;  // GCR::initialise src/GCR.h:31
    gcr->nrow = A->dim;
    return gcr_state_set_operator(gcr->gcr, A);
}

int mgcr_gcr_set_param(mgcr_op_t gcr, const mgcr_gcr_param *param) {
    MGCR_CHECK(gcr && param && gcr->kind == OP_GCR, MGCR_ERR_INVALID, "mgcr_gcr_set_param: not a GCR operator");
    LOCK();
    return gcr_state_set_param(gcr->gcr, param);
}

int mgcr_gcr_solve_op(mgcr_op_t gcr, mgcr_vec_t rhs, mgcr_vec_t x, double *hist, int32_t hist_cap, int32_t *n_iter,
                      int32_t *converged) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(gcr && rhs && x && gcr->kind == OP_GCR, MGCR_ERR_INVALID, "mgcr_gcr_solve_op: bad argument");
    MGCR_CHECK(rhs->n == gcr->dim, MGCR_ERR_INVALID, "Field dimension does not match with Operator!");
    MGCR_CHECK(x->n == gcr->dim, MGCR_ERR_INVALID, "x dimension does not match with Operator!");
    MGCR_CHECK(rhs->d != x->d, MGCR_ERR_INVALID, "rhs and x must be different Fields");
    LOCK();
    int it = 0, conv = 0;
    const bool xz = x->zero_known;
    int rc = gcr_run(gcr->gcr, rhs->d, x->w(), false, hist, hist_cap, &it, &conv, xz);
    if (n_iter) *n_iter = it;
    if (converged) *converged = conv;
    return rc;
}

int mgcr_gcr_set_x0(mgcr_op_t gcr, mgcr_vec_t x0) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(gcr && gcr->kind == OP_GCR, MGCR_ERR_INVALID, "mgcr_gcr_set_x0: not a GCR operator");
    LOCK();
    return gcr_state_set_x0(gcr->gcr, x0 ? x0->d : nullptr, x0 ? x0->n : 0);
}

int mgcr_set_small_solve_rows(int64_t rows) {
    MGCR_CHECK(rows >= 0, MGCR_ERR_INVALID, "rows must be >= 0");
    gcr_small_set_limit(rows);
    return MGCR_OK;
}

int mgcr_gcr_last_profile(double *phase_ms_total, int32_t *n_iter, int32_t *fused) {
    MGCR_CHECK(phase_ms_total && n_iter && fused, MGCR_ERR_INVALID, "null argument");
    int n = 0, f = 0;
    gcr_last_profile(phase_ms_total, &n, &f);
    *n_iter = n;
    *fused = f;
    return MGCR_OK;
}

int mgcr_bench_op_apply(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y, int32_t reps, double *ms_avg) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(op && x && y && reps > 0 && ms_avg, MGCR_ERR_INVALID, "mgcr_bench_op_apply: bad argument");
    MGCR_REFUSE_MULTI_DIRAC(op, "mgcr_bench_op_apply");
    MGCR_REFUSE_EVENODD_MULTI(op, "mgcr_bench_op_apply");
    LOCK();
    Context &c = ctx();
    MGCR_TRY(mgcr_op_apply(op, x, y));  // warm-up (and argument checks)
    MGCR_HIP(hipEventRecord(c.ev0, c.stream));
    for (int i = 0; i < reps; i++) MGCR_TRY(op_apply_raw(op, x->d, y->w(), x->n));
    MGCR_HIP(hipEventRecord(c.ev1, c.stream));
    MGCR_HIP(hipEventSynchronize(c.ev1));
    float ms = 0.f;
    MGCR_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    *ms_avg = (double)ms / reps;
    return MGCR_OK;
}

// ---- blocks of k Fields: k-wide apply (spmm.hip), batched GCR (gcr_multi.hip) ------------------------------------------
extern "C++" int mgcr::op_apply_multi_checks(mgcr_op_t op, mgcr_mvec_t x, mgcr_mvec_t y, const char *who) {   // (C++ linkage: internal, not part of the ABI)
    MGCR_CHECK(op && x && y, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_REFUSE_EVENODD(op, who);
    MGCR_REFUSE_GCR32(op, who);
    MGCR_CHECK(op->kind != OP_GCR && op->kind != OP_MG, MGCR_ERR_UNSUPPORTED, "%s: GCR and MG objects cannot be applied to a block of Fields", who);
    const Op *b0 = op_matrix(op);
    MGCR_CHECK(!op->dist && !op->comm && !b0->dist && !b0->comm, MGCR_ERR_UNSUPPORTED, "%s: distributed operators are not supported", who);
    MGCR_CHECK(x->n == op->dim, MGCR_ERR_INVALID, "Sparse matrix dimension does not match Field dimension!");
    const int64_t nrow = op->nrow ? op->nrow : op->dim;
    MGCR_CHECK(y->n == nrow, MGCR_ERR_INVALID, "output block has %lld rows, operator has %lld", (long long)y->n, (long long)nrow);
    MGCR_CHECK(x->k == y->k, MGCR_ERR_INVALID, "%s: input has %d columns, output has %d", who, (int)x->k, (int)y->k);
    MGCR_CHECK(op->kind != OP_DIRAC_MULTI || x->k == op->nk, MGCR_ERR_INVALID, "%s: the MultiDiracOp carries %d hopping parameters, the block has %d columns",
               who, op->nk, (int)x->k);
    MGCR_CHECK(op->kind != OP_DIRAC_EO_MULTI || x->k == op->nk, MGCR_ERR_INVALID,
               "%s: the MultiEvenOddDiracOp carries %d hopping parameters, the block has %d columns", who, op->nk, (int)x->k);
    MGCR_CHECK(x != y && (x->d != y->d || !x->d), MGCR_ERR_INVALID, "%s: input and output must be different blocks", who);
    return MGCR_OK;
}

int mgcr_op_apply_multi(mgcr_op_t op, mgcr_mvec_t x, mgcr_mvec_t y) {
    MGCR_TRY(require_ctx());
    MGCR_TRY(op_apply_multi_checks(op, x, y, "mgcr_op_apply_multi"));
    LOCK();
    return op_apply_multi_raw(op, x->d, y->d, x->n, x->k);
}

int mgcr_bench_op_apply_multi(mgcr_op_t op, mgcr_mvec_t x, mgcr_mvec_t y, int32_t reps, double *ms_avg) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(reps > 0 && ms_avg, MGCR_ERR_INVALID, "mgcr_bench_op_apply_multi: bad argument");
    MGCR_TRY(op_apply_multi_checks(op, x, y, "mgcr_bench_op_apply_multi"));
    LOCK();
    Context &c = ctx();
    MGCR_TRY(op_apply_multi_raw(op, x->d, y->d, x->n, x->k));  // warm-up
    MGCR_HIP(hipEventRecord(c.ev0, c.stream));
    for (int i = 0; i < reps; i++) MGCR_TRY(op_apply_multi_raw(op, x->d, y->d, x->n, x->k));
    MGCR_HIP(hipEventRecord(c.ev1, c.stream));
    MGCR_HIP(hipEventSynchronize(c.ev1));
    float ms = 0.f;
    MGCR_HIP(hipEventElapsedTime(&ms, c.ev0, c.ev1));
    *ms_avg = (double)ms / reps;
    return MGCR_OK;
}

int mgcr_gcr_solve_multi(mgcr_op_t A, const mgcr_gcr_param *param, mgcr_mvec_t rhs, mgcr_mvec_t x, double *hist, int32_t hist_cap,
                         int32_t *n_iter, int32_t *converged) {
    MGCR_TRY(require_ctx());
    MGCR_CHECK(A && param && rhs && x, MGCR_ERR_INVALID, "mgcr_gcr_solve_multi: null argument");
    MGCR_REFUSE_EVENODD(A, "mgcr_gcr_solve_multi");
    MGCR_REFUSE_GCR32(A, "mgcr_gcr_solve_multi");
    MGCR_CHECK(param->truncation >= 0 && param->restart >= 0 && param->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_CHECK(param->truncation == 0, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: truncation mode is not supported (restart mode only)");
    MGCR_CHECK(param->restart != 0, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: restart mode only (restart != 0)");
    MGCR_CHECK(!param->left_precond, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: a left preconditioner is not supported");
    MGCR_CHECK(!param->right_precond || param->flexible, MGCR_ERR_UNSUPPORTED,
               "mgcr_gcr_solve_multi: a right preconditioner is supported in flexible mode only (set flexible = 1)");
    MGCR_CHECK(!param->flexible || param->right_precond, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: flexible without a right preconditioner is not supported");
    MGCR_CHECK(!param->profile_spmv, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: profile_spmv is not supported");
    MGCR_CHECK(A->kind != OP_GCR && A->kind != OP_MG, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: the operator must be a matrix");
    {
        const Op *b0 = op_matrix(A);
        MGCR_CHECK(!A->dist && !A->comm && !b0->dist && !b0->comm, MGCR_ERR_UNSUPPORTED, "mgcr_gcr_solve_multi: distributed operators are not supported");
    }
    MGCR_CHECK(rhs->n == A->dim, MGCR_ERR_INVALID, "Field dimension does not match with Operator!");
    MGCR_CHECK(x->n == A->dim, MGCR_ERR_INVALID, "x dimension does not match with Operator!");
    MGCR_CHECK((A->nrow ? A->nrow : A->dim) == A->dim, MGCR_ERR_INVALID, "mgcr_gcr_solve_multi: the operator must be square");
    MGCR_CHECK(rhs->k == x->k, MGCR_ERR_INVALID, "mgcr_gcr_solve_multi: rhs has %d columns, x has %d", (int)rhs->k, (int)x->k);
    MGCR_CHECK(rhs != x && (rhs->d != x->d || !x->d), MGCR_ERR_INVALID, "rhs and x must be different blocks");
    MGCR_CHECK(A->kind != OP_DIRAC_MULTI || x->k == A->nk, MGCR_ERR_INVALID,
               "mgcr_gcr_solve_multi: the MultiDiracOp carries %d hopping parameters, the blocks have %d columns", A->nk, (int)x->k);
    MGCR_CHECK(A->kind != OP_DIRAC_EO_MULTI || x->k == A->nk, MGCR_ERR_INVALID,
               "mgcr_gcr_solve_multi: the MultiEvenOddDiracOp carries %d hopping parameters, the blocks have %d columns", A->nk, (int)x->k);
    if (mgcr_op_t M = param->right_precond) {   // flexible: a square low-precision GCR, or whatever mgcr_op_apply_multi takes, on dim rows
        const char *who = "mgcr_gcr_solve_multi: right_precond";
        if (M->kind == OP_GCR32) {
            MGCR_TRY(gcr32_multi_slot_check(M, A->dim, who));
        } else {
            MGCR_CHECK(M->kind != OP_DIRAC_MULTI && M->kind != OP_DIRAC_EO_MULTI, MGCR_ERR_UNSUPPORTED,
                       "%s: an operator with one hopping parameter per column has no single-Field counterpart in the slot", who);
            mgcr_mvec_s out;   // the shape M would write: the checks of mgcr_op_apply_multi, nothing is applied
            out.n = M->nrow ? M->nrow : M->dim;
            out.k = rhs->k;
            MGCR_TRY(op_apply_multi_checks(M, rhs, &out, who));
            MGCR_CHECK(out.n == A->dim, MGCR_ERR_INVALID, "%s: the preconditioner must be square, it has %lld rows", who, (long long)out.n);
        }
    }
    LOCK();
    return gcr_multi_run(A, *param, rhs->d, x->d, x->n, x->k, hist, hist_cap, n_iter, converged);
}

int mgcr_gcr_solve_queue(mgcr_op_t A, const mgcr_gcr_param *param, int32_t width, int32_t nsys, const mgcr_vec_t *rhs, const mgcr_vec_t *x,
                         const double *k_ri, double *hist, int32_t hist_cap, int32_t *n_iter, int32_t *converged) {
    const char *who = "mgcr_gcr_solve_queue";
    MGCR_TRY(require_ctx());
    MGCR_CHECK(A && param && rhs && x, MGCR_ERR_INVALID, "%s: null argument", who);
    MGCR_REFUSE_EVENODD(A, who);
    MGCR_REFUSE_EVENODD_MULTI(A, who);
    MGCR_REFUSE_GCR32(A, who);
    MGCR_CHECK(param->truncation >= 0 && param->restart >= 0 && param->max_iter >= 0, MGCR_ERR_INVALID, "negative GCR parameter");
    MGCR_CHECK(param->truncation == 0, MGCR_ERR_UNSUPPORTED, "%s: truncation mode is not supported (restart mode only)", who);
    MGCR_CHECK(param->restart != 0, MGCR_ERR_UNSUPPORTED, "%s: restart mode only (restart != 0)", who);
    MGCR_CHECK(!param->left_precond && !param->right_precond, MGCR_ERR_UNSUPPORTED, "%s: preconditioners are not supported", who);
    MGCR_CHECK(!param->flexible && !param->profile_spmv, MGCR_ERR_UNSUPPORTED, "%s: flexible / profile_spmv are not supported", who);
    MGCR_CHECK(A->kind != OP_GCR && A->kind != OP_MG, MGCR_ERR_UNSUPPORTED, "%s: the operator must be a matrix", who);
    {
        const Op *b0 = op_matrix(A);
        MGCR_CHECK(!A->dist && !A->comm && !b0->dist && !b0->comm, MGCR_ERR_UNSUPPORTED, "%s: distributed operators are not supported", who);
    }
    if (k_ri) {
        MGCR_CHECK(A->kind == OP_CSR, MGCR_ERR_INVALID, "%s: with hopping parameters the operator must be the plain Sparse D of 1 - k D", who);
        MGCR_CHECK(A->csr.nrow == A->csr.ncol, MGCR_ERR_INVALID, "%s: matrix must be square", who);
    } else {
        MGCR_CHECK(A->kind != OP_DIRAC_MULTI, MGCR_ERR_UNSUPPORTED,
                   "%s: a MultiDiracOp's width is that of a block; pass its Sparse and the hopping parameters (k_ri) instead", who);
    }
    MGCR_CHECK(width >= 1 && width <= MV_MAX_K, MGCR_ERR_INVALID, "%s: width = %d slots, 1 .. %d are supported", who, (int)width, MV_MAX_K);
    MGCR_CHECK(nsys >= 1, MGCR_ERR_INVALID, "%s: nsys = %d systems", who, (int)nsys);
    MGCR_CHECK((A->nrow ? A->nrow : A->dim) == A->dim, MGCR_ERR_INVALID, "%s: the operator must be square", who);
    std::vector<const void *> xs, bs;
    for (int32_t s = 0; s < nsys; s++) {
        MGCR_CHECK(rhs[s] && x[s], MGCR_ERR_INVALID, "%s: system %d has a null Field", who, (int)s);
        MGCR_CHECK(rhs[s]->n == A->dim, MGCR_ERR_INVALID, "Field dimension does not match with Operator!");
        MGCR_CHECK(x[s]->n == A->dim, MGCR_ERR_INVALID, "x dimension does not match with Operator!");
        xs.push_back(x[s]->d);
        bs.push_back(rhs[s]->d);
    }
    if (A->dim > 0) {   // the x Fields are written while other systems still read their right-hand sides
        std::sort(xs.begin(), xs.end());
        std::sort(bs.begin(), bs.end());
        MGCR_CHECK(std::adjacent_find(xs.begin(), xs.end()) == xs.end(), MGCR_ERR_INVALID, "%s: the x Fields must be pairwise distinct", who);
        for (const void *q : xs)
            MGCR_CHECK(!std::binary_search(bs.begin(), bs.end(), q), MGCR_ERR_INVALID, "%s: an x Field is also a right-hand side", who);
    }
    std::vector<cplx> ks;
    if (k_ri) {
        ks.resize((size_t)nsys);
        for (int32_t s = 0; s < nsys; s++) {
            MGCR_CHECK(k_ri[2 * s] != 0. || k_ri[2 * s + 1] != 0., MGCR_ERR_INVALID, "%s: k[%d] is zero (No k value supplied for Dirac Operator!)", who, (int)s);
            ks[(size_t)s] = make_double2(k_ri[2 * s], k_ri[2 * s + 1]);
        }
    }
    LOCK();
    std::vector<const cplx *> bp((size_t)nsys);
    std::vector<cplx *> xp((size_t)nsys);
    for (int32_t s = 0; s < nsys; s++) {
        bp[(size_t)s] = rhs[s]->d;
        xp[(size_t)s] = x[s]->w();
    }
    return gcr_queue_run(A, *param, width, nsys, bp.data(), xp.data(), k_ri ? ks.data() : nullptr, A->dim, hist, hist_cap, n_iter, converged);
}

}  // extern "C"
