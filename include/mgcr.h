/* mgcr.h — C ABI of libmgcr_hip.so: the MI355X (gfx950) implementation of the multigrid-
 * preconditioned GCR inner loop (SpMV + MG V-cycle pieces + GCR orthogonalisation).
 *
 * The reference (jing2li/MGPreconditionedGCR @ 2024_10_08) has no FFI: its seam is the C++
 * virtual `Operator<num_type>` plus `Field<num_type>` and the `*_Param` structs.  Every entry
 * point below names the reference interface it replaces (paths relative to the reference root);
 * include/mgcr/ *.h re-creates those C++ classes on top of this ABI.
 *
 * Conventions
 *  - plain C types only; complex data is interleaved (re,im) doubles ("ri"), i.e. layout-
 *    compatible with std::complex<double>[] (src/Fields.h:70, src/Operator.h:97);
 *  - every function returns an int status (MGCR_OK = 0); mgcr_last_error() gives the message of
 *    the last failure on the calling thread.  Nothing aborts (the reference asserts/exit(1)s,
 *    src/Fields.h:14,279-283 — the C++ shim turns a non-zero status back into that behaviour);
 *  - host arrays passed in are copied, never adopted; handles are opaque and destroyed explicitly;
 *  - one process drives one GPU (mgcr_init(device)); the library is thread-compatible: entry
 *    points serialise on an internal mutex, so an operator may be applied from several host
 *    threads (the reference does that inside its OpenMP set-up loops, src/MG.h:206-278);
 *  - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *    MGCR_ERR_NO_DEVICE.
 */
#ifndef MGCR_H
#define MGCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGCR_OK 0
#define MGCR_ERR_INVALID 1      /* bad argument (size mismatch, null handle, ...) */
#define MGCR_ERR_NO_DEVICE 2    /* no HIP device / mgcr_init not called */
#define MGCR_ERR_HIP 3          /* a HIP runtime call failed */
#define MGCR_ERR_ALLOC 4
#define MGCR_ERR_IO 5
#define MGCR_ERR_COMM 6
#define MGCR_ERR_UNSUPPORTED 7

typedef struct mgcr_vec_s *mgcr_vec_t; /* device-resident Field   (src/Fields.h:29-71)   */
typedef struct mgcr_op_s *mgcr_op_t;   /* device-resident Operator (src/Operator.h:16-29) */
typedef struct mgcr_mvec_s *mgcr_mvec_t; /* device-resident block of k Fields (multi-RHS; no reference counterpart) */

/* ---- context ------------------------------------------------------------------------------ */
int mgcr_init(int device);
int mgcr_finalize(void);
const char *mgcr_last_error(void);
const char *mgcr_version(void);
/* name, CU count and total memory of the active device */
int mgcr_device_info(char *name, int name_cap, int *n_cu, int64_t *mem_bytes);
/* blocks until all work queued by this library has finished */
int mgcr_synchronize(void);

/* ---- Field: src/Fields.h ------------------------------------------------------------------- */
int mgcr_vec_create(int64_t n, mgcr_vec_t *out);                   /* Field(dims,ndim)   :77-80  */
int mgcr_vec_destroy(mgcr_vec_t v);                                /* ~Field             :186-190 */
int64_t mgcr_vec_size(mgcr_vec_t v);                               /* field_size         :120-123 */
int mgcr_vec_upload(mgcr_vec_t v, const double *host_ri);          /* Field(dims,ndim,init) :83-89 */
int mgcr_vec_download(mgcr_vec_t v, double *host_ri);              /* val_at             :163-168 */
int mgcr_vec_copy(mgcr_vec_t dst, mgcr_vec_t src);                 /* operator=          :256-286 */
int mgcr_vec_zero(mgcr_vec_t v);                                   /* set_zero           :137-145 */
int mgcr_vec_set_constant(mgcr_vec_t v, const double c_ri[2]);     /* set_constant       :146-151 */
/* deterministic repo-owned RHS on the grid of init_rand (:125-135) — splitmix64, not libc rand */
int mgcr_vec_fill_rhs(mgcr_vec_t v, uint64_t seed, int64_t global_offset);
int mgcr_dot(mgcr_vec_t a, mgcr_vec_t b, double out_ri[2]);        /* dot: sum conj(a)b  :216-226 */
int mgcr_norm2(mgcr_vec_t a, double *out);                         /* squarednorm        :228-235 */
/* out = a + alpha*b   (operator+ / operator- / operator* fused)                 :192-214,245-253 */
int mgcr_add_scaled(mgcr_vec_t out, mgcr_vec_t a, const double alpha_ri[2], mgcr_vec_t b);
int mgcr_axpy(const double alpha_ri[2], mgcr_vec_t x, mgcr_vec_t y); /* y += alpha*x  (+=  :288-297) */
int mgcr_scale(mgcr_vec_t v, const double alpha_ri[2]);            /* operator*          :245-253 */
int mgcr_normalise(mgcr_vec_t v);                                  /* normalise          :237-243 */
/* gamma5 :310-339  out[index with spinor 0<->2, 1<->3] = in[index]; `inner` = product of the mesh dimensions after the
 * (4-entry) spinor dimension */
int mgcr_vec_gamma5(mgcr_vec_t in, mgcr_vec_t out, int64_t inner);

/* ---- multi-vector: a block of k Fields, 1 <= k <= 16 (new: the reference works on one right-hand side at a time) ----
 * Device layout: row-major with the columns INTERLEAVED, element (row i, column j) at data[i * k + j] — the k values an
 * operator gathers for one column index are contiguous (k = 8: one 128-byte line), and a matrix is streamed once for all
 * k products (mgcr_op_apply_multi).  Host arrays hold k contiguous columns, [k][n] interleaved (re, im); the transposition
 * runs on the device. */
int mgcr_mvec_create(int64_t n, int32_t k, mgcr_mvec_t *out);      /* k outside 1 .. 16: MGCR_ERR_INVALID */
int mgcr_mvec_destroy(mgcr_mvec_t v);
int64_t mgcr_mvec_size(mgcr_mvec_t v);                             /* n: rows = entries per column */
int32_t mgcr_mvec_ncols(mgcr_mvec_t v);                            /* k */
int mgcr_mvec_zero(mgcr_mvec_t v);
int mgcr_mvec_upload(mgcr_mvec_t v, const double *host_ri);        /* host: [k][n][2] */
int mgcr_mvec_download(mgcr_mvec_t v, double *host_ri);
int mgcr_mvec_set_column(mgcr_mvec_t v, int32_t j, mgcr_vec_t src);  /* column j = src (device-side pack) */
int mgcr_mvec_get_column(mgcr_mvec_t v, int32_t j, mgcr_vec_t dst);  /* dst = column j (device-side unpack) */
/* k dot products (conj on a) / squared norms in ONE pass over a and b: out_ri[2 j], out_ri[2 j + 1] = <a_j, b_j>, out[j] = |a_j|^2.
 * Same rows per thread, same summation tree and fold as mgcr_dot / mgcr_norm2: the value of column j has the bits of
 * mgcr_dot / mgcr_norm2 on that column held in a Field. */
int mgcr_mvec_dot(mgcr_mvec_t a, mgcr_mvec_t b, double *out_ri);
int mgcr_mvec_norm2(mgcr_mvec_t a, double *out);
int mgcr_mvec_axpy(const double *alpha_ri, mgcr_mvec_t x, mgcr_mvec_t y);  /* y_j += alpha_j x_j, alpha_ri: [k][2] */

/* ---- Operators: src/Operator.h, src/HierarchicalSparse.h ---------------------------------- */
/* Sparse<long> (CSR, int64 indices as the reference stores them, src/Operator.h:56-101).  The
 * device copy is an ELL slab (column-major, int32 columns) plus a CSR tail for long rows. */
int mgcr_csr_create(int64_t nrow, int64_t ncol, const int64_t *rowptr, const int64_t *col,
                    const double *val_ri, mgcr_op_t *out);
/* DiracOp = 1 - k D (src/Operator.h:104-122,569-575): a view on `csr` that applies
 * y = x - k*(D x) with the shift fused into the SpMV epilogue.  Borrows `csr` (as the reference
 * borrows its Sparse*). */
int mgcr_dirac_create(mgcr_op_t csr, const double k_ri[2], mgcr_op_t *out);
int mgcr_dirac_set_k(mgcr_op_t dirac, const double k_ri[2]);       /* set_k src/Operator.h:116 */
/* MultiDiracOp: 1 - k_j D on column j of a block of exactly k Fields (hopping-parameter scans: one D, one stream of the matrix,
 * a ladder of k_j; no reference counterpart — test_kcritical, src/main.cpp:696-741, builds one DiracOp per value).  Borrows `csr`
 * as mgcr_dirac_create does.  k_ri: [k][2], 1 <= k <= 16; a zero k_j, k outside 1 .. 16: MGCR_ERR_INVALID; a distributed
 * Sparse: MGCR_ERR_UNSUPPORTED.  ONLY mgcr_op_apply_multi and mgcr_gcr_solve_multi take it, with blocks of exactly k columns
 * (any other width: MGCR_ERR_INVALID); the entry points that work on one Field (mgcr_op_apply, mgcr_gcr_solve, mgcr_gcr_create,
 * mgcr_gcr_set_operator, mgcr_mg_create, mgcr_bench_op_apply) answer MGCR_ERR_UNSUPPORTED.  The queries (mgcr_op_dim / nrow /
 * nnz / stored_bytes / storage_format / ell_layout / xr_fuse_kind) answer for the Sparse, as for a DiracOp.
 * Rule 1: column j of mgcr_op_apply_multi(MultiDiracOp(D, ks), X) is BIT-IDENTICAL to mgcr_op_apply of DiracOp(D, ks[j]) on
 * column j of X.
 * Rule 2: history, iteration count, convergence flag and x of column j of mgcr_gcr_solve_multi are BIT-IDENTICAL to
 * mgcr_gcr_solve with DiracOp(D, ks[j]) on column j alone, under the conditions mgcr_gcr_solve_multi states (default options,
 * mgcr_op_xr_fuse_kind 0 or 1, more rows than the small-solve limit).  The columns of a scan stop at different steps; a
 * stopped column is frozen as in every batched solve.
 * mgcr_dirac_multi_set_k replaces all k values (same count).  They travel in the kernel arguments of each launch: the new
 * values hold for every later call and never for work already enqueued. */
int mgcr_dirac_multi_create(mgcr_op_t csr, int32_t k, const double *k_ri /* [k][2] */, mgcr_op_t *out);
int mgcr_dirac_multi_set_k(mgcr_op_t op, const double *k_ri /* [k][2] */);
/* EvenOddDiracOp: the even-odd (red-black) preconditioned 1 - k D (no reference counterpart — test_kcritical, src/main.cpp:696-741,
 * solves the full system).  D must be a pure hopping matrix: square, NO diagonal, every entry joining an even row to an odd one.
 * Then A x = b reduces to the Schur system on the even half,
 *     S x_e = bhat_e,   S = 1 - k^2 D_eo D_oe,   bhat_e = b_e + k D_eo b_o,   x_o = b_o + k D_oe x_e,
 * and the operator made here IS S: an Operator on Fields of n_e entries (mgcr_op_dim = mgcr_op_nrow = n_e, mgcr_op_nnz = that of
 * D).  Operators with a diagonal (Poisson, a clover term) are out of scope, and so is distributed use.
 * mgcr_eo_create COPIES the matrix (host CSR, int64 indices).  parity: [n] 0 even / 1 odd, or NULL — the graph of D + D^T is then
 * two-coloured breadth first, components in order of their smallest row, that row (an isolated or empty row included) even.
 * Given or computed, the parity is checked: an entry that joins two rows of equal colour (a diagonal entry, an odd cycle, a wrong
 * caller bit) is MGCR_ERR_INVALID, and the message names the first such (row, column).  k = 0: MGCR_ERR_INVALID, here and in
 * mgcr_eo_set_k (DiracOp's "No k value supplied").
 * Layout: even[] / odd[] are the ascending full-system rows of each colour; D_eo (n_e x n_o) and D_oe (n_o x n_e) keep their rows
 * in list order, renumber the columns into the other list and keep a row's entries in stored order; each half is a Sparse of its
 * own in whatever storage form mgcr_csr_create would choose for it.  mgcr_eo_half_op lends them (0: D_eo, 1: D_oe; owned by the
 * operator like the levels mgcr_mg_level_op lends, not to be destroyed).
 * mgcr_eo_split / mgcr_eo_merge move a full Field to / from its (even, odd) halves; mgcr_eo_prepare forms bhat_e from b;
 * mgcr_eo_reconstruct forms x_o from b and x_e and merges.  mgcr_eo_solve = prepare, mgcr_gcr_solve(S, param, bhat_e, x_e),
 * reconstruct (the operator keeps that solver's state and work Fields between calls); x_e is the even half of x_full on entry and use_x0 behaves as documented for mgcr_gcr_solve (the reference's
 * r0 = b quirk applies to the EVEN system); history, iteration count and convergence flag are the Schur solve's, relative to
 * |bhat_e|: the full system's true residual |(1 - k D) x - b| / |b| is hist[last] |bhat_e| / |b|, its odd half is rounding only.
 * Accepted by: mgcr_op_apply (Fields of n_e entries), mgcr_bench_op_apply, mgcr_gcr_solve, mgcr_gcr_create /
 * mgcr_gcr_set_operator, and as a preconditioner slot.  MGCR_ERR_UNSUPPORTED from: mgcr_op_apply_multi, mgcr_gcr_solve_multi,
 * mgcr_gcr_solve_queue, mgcr_mg_create and the storage queries (stored_bytes / storage_format / ell_layout / xr_fuse_kind /
 * halo_kind; ask the halves).  A Field of the wrong length: MGCR_ERR_INVALID, on every entry point.
 * Rule 1 (apply): through the public entry points, BIT-IDENTICAL are
 *     mgcr_op_apply(eo, x, y)            and  t = D_oe(x); u = D_eo(t); mgcr_add_scaled(y, x, -k2, u)   (k2 = k k, un-fused),
 *     mgcr_eo_prepare                    and  mgcr_add_scaled(bhat_e, b_e, +k, D_eo(b_o)),
 *     the odd half of mgcr_eo_reconstruct  and  mgcr_add_scaled(x_o, b_o, +k, D_oe(x_e)),
 * with the half operators of mgcr_eo_half_op (the library is built without FP contraction: a - c s and a + (-c) s have the same bits).
 * Rule 2 (solve): history, iteration count, convergence flag and x of a GCR solve on the operator are BIT-IDENTICAL with the
 * option fused_apply on and off.  On: where D_eo is stored one thread per row, the second stage of each step's apply also takes
 * the step's beta dot products (one launch less per step); off: two plain applies, then the dot products.
 * A GCR solve on this operator always runs the multi-kernel path: no one-launch solve, step or start, no graph replay.
 * mgcr_eo_set_k: the values travel in the kernel arguments of each launch — the new k holds for every later call and never for
 * work already enqueued. */
int mgcr_eo_create(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri,
                   const int8_t *parity /* [n] 0 even, 1 odd; NULL: two-colour */, const double k_ri[2], mgcr_op_t *out);
int mgcr_eo_set_k(mgcr_op_t eo, const double k_ri[2]);
int mgcr_eo_info(mgcr_op_t eo, int64_t *n, int64_t *n_even, int64_t *n_odd);
int mgcr_eo_parity(mgcr_op_t eo, int8_t *parity /* [n] */);
int mgcr_eo_half_op(mgcr_op_t eo, int32_t which /* 0: D_eo, 1: D_oe */, mgcr_op_t *borrowed);
int mgcr_eo_split(mgcr_op_t eo, mgcr_vec_t full, mgcr_vec_t even, mgcr_vec_t odd);
int mgcr_eo_merge(mgcr_op_t eo, mgcr_vec_t even, mgcr_vec_t odd, mgcr_vec_t full);
int mgcr_eo_prepare(mgcr_op_t eo, mgcr_vec_t b_full, mgcr_vec_t bhat_even);
int mgcr_eo_reconstruct(mgcr_op_t eo, mgcr_vec_t b_full, mgcr_vec_t x_even, mgcr_vec_t x_full);
/* (mgcr_eo_solve is declared below, with the solver entry points) */
/* EvenOddDiagDiracOp / EvenOddSparse, the even-odd Schur solve for operators with a SITE diagonal (Poisson, a mass term, twisted
 * mass, a shift): one complex number per row, so the diagonal blocks are scalars and their inverse is element-wise.  Write the full
 * operator as A = diag(a) - c H with H the stored off-diagonal part; H must be two-colourable exactly as for mgcr_eo_create, and
 * diagonal entries are ignored by the colouring and by its check (an odd cycle or a wrong caller bit is still MGCR_ERR_INVALID
 * with the entry named).
 *     Dirac form  (k_ri != NULL):  A = 1 - k D, D may store a diagonal d:   a = (1, 0) - k d,  c = k;   k = 0: MGCR_ERR_INVALID;
 *     matrix form (k_ri == NULL):  A = M itself:                            a = d,             c = -1.
 * d of a row = its stored diagonal entries added in stored order, 0 if it has none.  The Schur system on the even half is
 *     S x_e = bhat_e,  S = diag(a_e) - c^2 H_eo diag(1/a_o) H_oe,  bhat_e = b_e + c H_eo (b_o / a_o),  x_o = (b_o + c H_oe x_e) / a_o.
 * Complex products are (ar br - ai bi, ar bi + ai br), 1/a = (ar / den, -ai / den) with den = ar ar + ai ai, nothing is fused, and
 * c2 = c c and cn = -c are formed once on the host.  a_e may contain zeros; an exactly zero or non-finite 1/a_o is
 * MGCR_ERR_INVALID and the message names the full-system row.
 * mgcr_eo_create_diag makes an EvenOddDiracOp (mgcr_op_nnz counts the whole matrix, diagonal included): every entry point that
 * takes the operator of mgcr_eo_create takes this one — mgcr_op_apply, mgcr_gcr_solve, mgcr_gcr_create / mgcr_gcr_set_operator,
 * the preconditioner slot, mgcr_eo_split / merge / prepare / reconstruct / solve, mgcr_eo_info / parity / half_op (the halves lent
 * are the OFF-DIAGONAL halves H_eo, H_oe).  mgcr_eo_diag downloads a_e [n_e][2] and 1/a_o [n_o][2]; for an operator made by
 * mgcr_eo_create both are all ones.  mgcr_eo_set_k on the Dirac form recomputes a and 1/a_o in stream order (work already
 * enqueued keeps the old values); the singular check runs on the host first and a refused k leaves the operator at its previous
 * k.  On the matrix form mgcr_eo_set_k is MGCR_ERR_INVALID.
 * Refused with MGCR_ERR_UNSUPPORTED: mgcr_eo_multi_create and mgcr_eo_solve_queue on an operator that carries a diagonal (the
 * diagonal 1 - k_j d would be per column), besides everything mgcr_eo_create's operator is refused by.
 * Rule 1d (apply): with a_e and inv_o = 1/a_o from mgcr_eo_diag, the halves from mgcr_eo_half_op, and the element-wise products (.)
 * formed on the host as real and imaginary parts with separate real operations, BIT-IDENTICAL are
 *     mgcr_op_apply(eo, x, y)                and  u = H_oe(x); t = inv_o (.) u; v = H_eo(t); y = a_e (.) x - c2 v,
 *     mgcr_eo_prepare                        and  b_e - cn H_eo(inv_o (.) b_o),
 *     the odd half of mgcr_eo_reconstruct    and  inv_o (.) (b_o - cn H_oe(x_e));
 * the even half of mgcr_eo_reconstruct is x_e itself.
 * Rule 2d (solve): history, iteration count, convergence flag and x of a GCR solve on the operator are BIT-IDENTICAL with the
 * option fused_apply on and off.  On: where H_eo is stored one thread per row, stage 2 of each step's apply takes the step's beta
 * dot products (the counter "evenodd_diag_fused_steps"; "evenodd_fused_steps" does not move).
 * Rule 3d (no diagonal): a matrix without any stored diagonal entry, made through mgcr_eo_create_diag in Dirac form, gives exactly
 * what mgcr_eo_create gives for apply, prepare, reconstruct and solve — it IS that operator, on that code path. */
int mgcr_eo_create_diag(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri,
                        const int8_t *parity /* [n] 0 even, 1 odd; NULL: two-colour */, const double *k_ri /* [2]; NULL: matrix form */,
                        mgcr_op_t *out);
int mgcr_eo_diag(mgcr_op_t eo, double *a_even_ri /* [n_e][2] */, double *inv_a_odd_ri /* [n_o][2] */);
/* EvenOddBlockDiracOp / EvenOddBlockSparse, the even-odd Schur solve for operators with a dense BLOCK PER SITE on the diagonal
 * (clover-type operators, a mass matrix, a local potential, block Poisson).  Sites are runs of bs consecutive rows: row r belongs
 * to site r / bs, n % bs == 0, 1 <= bs <= 16.  Write the full operator as A = B - c H: H the stored entries between different
 * sites, B block diagonal, one bs x bs complex block per site built from the stored entries inside the site.
 *     Dirac form  (k_ri != NULL):  A = 1 - k D:   B_s = I - k D_ss ((1, 0) - k d on the diagonal, (0, 0) - k d off it),  c = k;
 *     matrix form (k_ri == NULL):  A = M itself:  B_s = D_ss,                                                             c = -1.
 * Entry (i, j) of D_ss = the stored entries at that position added in stored order, 0 if none is stored.  The rows of a site
 * share one colour: the colouring runs on the SITE graph of H (as mgcr_eo_create colours rows), a caller parity [n] must be
 * constant inside every site, and the index lists stay ascending, so half-site s' occupies the half rows s' bs .. s' bs + bs - 1.
 *     S x_e = bhat_e,  S = B_e - c^2 H_eo B_o^-1 H_oe,  bhat_e = b_e + c H_eo (B_o^-1 b_o),  x_o = B_o^-1 (b_o + c H_oe x_e).
 * Complex products are (ar br - ai bi, ar bi + ai br), 1/a = (ar / den, -ai / den) with den = ar ar + ai ai, nothing is fused,
 * c2 = c c and cn = -c are formed once on the host, and a block-vector product (B (.) x)_i is B_i0 x_0, then + B_ij x_j for
 * j = 1 .. bs - 1 ascending, real and imaginary parts accumulated separately.  B_o^-1 is formed on the device by Gauss-Jordan
 * elimination with partial pivoting on [B | I]: for each pivot column p = 0 .. bs - 1 the row i >= p with the largest re^2 + im^2
 * in column p (the first maximum wins) is swapped into row p, piv = 1 / a_pp, every entry of row p is multiplied by piv, and every
 * other row i, with f = a_ip, becomes row_i - f (.) row_p entry by entry; the right half is then B^-1.
 * mgcr_eo_create_block makes an EvenOddDiracOp (mgcr_op_nnz counts the whole matrix): every entry point that takes the operator
 * of mgcr_eo_create_diag takes this one — mgcr_op_apply, mgcr_gcr_solve, mgcr_gcr_create / mgcr_gcr_set_operator, the
 * preconditioner slot, mgcr_eo_split / merge / prepare / reconstruct / solve, mgcr_eo_info / parity / half_op (the halves lent are
 * the INTER-SITE halves H_eo, H_oe).  mgcr_eo_block_info gives bs and the number of even and odd sites; mgcr_eo_block_diag
 * downloads B of the even sites [sites_e][bs][bs][2] and B^-1 of the odd sites [sites_o][bs][bs][2], row-major (for an operator
 * without blocks: bs = 1 and what mgcr_eo_diag gives).  On an operator with blocks mgcr_eo_diag is MGCR_ERR_INVALID.
 * mgcr_eo_set_k on the Dirac form recomputes the blocks in stream order (work already enqueued keeps the old ones); it inverts
 * into a spare buffer and the host reads one status word — ONE synchronisation per call — before the buffers are swapped, so a
 * refused k leaves the operator at its previous k, blocks included.  On the matrix form mgcr_eo_set_k is MGCR_ERR_INVALID.
 * MGCR_ERR_INVALID, with the entry, site or row named: bs outside 1 .. 16; n % bs != 0; k = 0; an odd cycle in the site graph (one
 * inter-site entry (row, column) on it is named); a caller parity that differs inside a site; a caller parity that gives both
 * ends of an inter-site entry one colour; an odd block whose elimination meets an exactly zero or non-finite pivot (den): the
 * message names the site and the full-system row of the pivot column — at creation and in mgcr_eo_set_k.  Even blocks may be
 * singular.
 * Refused with MGCR_ERR_UNSUPPORTED: mgcr_eo_multi_create and mgcr_eo_solve_queue on an operator with blocks (dense site blocks
 * would be per column), besides everything mgcr_eo_create's operator is refused by.
 * Rule 1b (blocks): what mgcr_eo_block_diag downloads is BIT-IDENTICAL to the entry-by-entry formulas and the elimination above.
 * Rule 2b (apply): with B_e and invB_o from mgcr_eo_block_diag, the halves from mgcr_eo_half_op, and the block products (.)
 * formed on the host in the stated order, BIT-IDENTICAL are
 *     mgcr_op_apply(eo, x, y)                and  y = B_e (.) x - c2 H_eo(invB_o (.) H_oe(x)),
 *     mgcr_eo_prepare                        and  b_e - cn H_eo(invB_o (.) b_o),
 *     the odd half of mgcr_eo_reconstruct    and  invB_o (.) (b_o - cn H_oe(x_e));
 * the even half of mgcr_eo_reconstruct is x_e itself.
 * Rule 3b (solve): history, iteration count, convergence flag and x of a GCR solve on the operator are BIT-IDENTICAL with the
 * option fused_apply on and off.  On: the last launch of each step's apply takes the step's beta dot products (the counter
 * "evenodd_block_fused_steps"; "evenodd_fused_steps" and "evenodd_diag_fused_steps" do not move).  mgcr_eo_solve equals
 * mgcr_eo_prepare + mgcr_gcr_solve on the operator + mgcr_eo_reconstruct, bit for bit.
 * Rule 4b (bs = 1): mgcr_eo_create_block with bs = 1 gives exactly what mgcr_eo_create_diag gives for apply, prepare,
 * reconstruct and solve — it IS that operator, on that code path ("evenodd_diag_fused_steps" moves, the block counters do not). */
int mgcr_eo_create_block(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, int32_t bs,
                         const int8_t *parity /* [n]; NULL: two-colour the sites */, const double *k_ri /* [2]; NULL: matrix form */,
                         mgcr_op_t *out);
int mgcr_eo_block_info(mgcr_op_t eo, int32_t *bs, int64_t *sites_even, int64_t *sites_odd);
int mgcr_eo_block_diag(mgcr_op_t eo, double *B_even_ri /* [sites_e][bs][bs][2], row-major */,
                       double *invB_odd_ri /* [sites_o][bs][bs][2] */);
/* MultiEvenOddDiracOp, even-odd hopping-parameter scans: the Schur complements S_j = 1 - k_j^2 D_eo D_oe on column j of a block of
 * exactly nk Fields of the even half (mgcr_op_dim = mgcr_op_nrow = n_e, mgcr_op_nnz = that of D).  The fewer steps of the even-odd
 * solve and the shared matrix stream and launches of the batched solve in one operator.  It BORROWS the two half matrices and the
 * index lists of `eo`, an EvenOddDiracOp, which must outlive it; nothing is copied or planned again, and eo's own k is not used.
 * k_ri: [nk][2], 1 <= nk <= 16.  nk outside 1 .. 16, a zero k_j ("No k value supplied"), an `eo` that is no EvenOddDiracOp:
 * MGCR_ERR_INVALID.  mgcr_eo_multi_set_k replaces all nk values.  The values and their squares (formed on the host, as
 * mgcr_eo_set_k forms its one) travel in the kernel arguments of each launch: they hold for every later call and never for work
 * already enqueued.
 * Accepted by: mgcr_op_apply_multi (blocks of n_e rows x nk columns), mgcr_bench_op_apply_multi, mgcr_gcr_solve_multi (the nk Schur
 * systems, under that entry point's restrictions), mgcr_op_destroy / dim / nrow / nnz, and the mgcr_eo_multi entry points: split,
 * merge, prepare and reconstruct are mgcr_eo_split ... mgcr_eo_reconstruct on blocks of nk columns (full blocks have n rows, even
 * ones n_e, odd ones n_o), and mgcr_eo_multi_solve = prepare, mgcr_gcr_solve_multi(S, param, Bhat_e, X_e), reconstruct, with X_e the
 * even half of X_full on entry and use_x0 as in mgcr_eo_solve; hist: [nk][hist_cap], row j relative to |bhat_e,j|; n_iter,
 * converged: [nk].  The operator keeps its work blocks (the batched solver's storage is the library's, see mgcr_gcr_solve_multi).
 * MGCR_ERR_UNSUPPORTED, with a message naming the kind, from: mgcr_op_apply, mgcr_bench_op_apply, mgcr_gcr_solve, mgcr_gcr_create,
 * mgcr_gcr_set_operator, mgcr_gcr_solve_queue, mgcr_mg_create and the storage queries (stored_bytes / storage_format / ell_layout /
 * xr_fuse_kind / halo_kind; ask the halves of `eo`).  A block of another width or length, blocks that alias: MGCR_ERR_INVALID.
 * The plain EvenOddDiracOp goes on refusing the block, queue and multigrid entry points.
 * Rule 1: column j of mgcr_op_apply_multi, mgcr_eo_multi_prepare, mgcr_eo_multi_reconstruct, mgcr_eo_multi_split and
 * mgcr_eo_multi_merge is BIT-IDENTICAL to mgcr_op_apply, mgcr_eo_prepare, mgcr_eo_reconstruct, mgcr_eo_split and mgcr_eo_merge on
 * column j with EvenOddDiracOp(D, k_j), in every storage form of the halves.
 * Rule 2: history, iteration count, convergence flag and x of column j of mgcr_gcr_solve_multi on the operator are BIT-IDENTICAL
 * to mgcr_gcr_solve on EvenOddDiracOp(D, k_j) with column j alone, and those of mgcr_eo_multi_solve to mgcr_eo_solve — at ANY size:
 * the single Schur solve never takes a one-workgroup or one-launch path, so the small-size exception of the MultiDiracOp's Rule 2
 * does not arise.  The batched cycle takes the beta dot products in passes of their own; the single solve's fused second stage
 * has their bits.
 * Ladders of more than 16 values, or of very unequal lengths, go through mgcr_eo_solve_queue (below, with the solver entry points).
 * Out of scope: distributed halves, operators with a diagonal. */
int mgcr_eo_multi_create(mgcr_op_t eo, int32_t nk, const double *k_ri /* [nk][2] */, mgcr_op_t *out);
int mgcr_eo_multi_set_k(mgcr_op_t op, const double *k_ri /* [nk][2] */);
int mgcr_eo_multi_split(mgcr_op_t op, mgcr_mvec_t full, mgcr_mvec_t even, mgcr_mvec_t odd);
int mgcr_eo_multi_merge(mgcr_op_t op, mgcr_mvec_t even, mgcr_mvec_t odd, mgcr_mvec_t full);
int mgcr_eo_multi_prepare(mgcr_op_t op, mgcr_mvec_t B_full, mgcr_mvec_t Bhat_even);
int mgcr_eo_multi_reconstruct(mgcr_op_t op, mgcr_mvec_t B_full, mgcr_mvec_t X_even, mgcr_mvec_t X_full);
/* (mgcr_eo_multi_solve is declared below, with the solver entry points) */
/* HierarchicalSparse<long,int> (block-CSR of dense bs x bs blocks, row-major inside a block,
 * src/HierarchicalSparse.h:22-48) from UNSORTED (block-row, block-col, block) triplets with the
 * constructor's semantics (:58-98): sorted by row*nbcol+col, duplicates of a pair kept and
 * summed at apply time. */
int mgcr_bcsr_create_from_triplets(int32_t nbrow, int32_t nbcol, int32_t bs, int32_t ntriplets,
                                   const int32_t *rows, const int32_t *cols, const double *blocks_ri,
                                   mgcr_op_t *out);
int mgcr_bcsr_create(int32_t nbrow, int32_t nbcol, int32_t bs, const int32_t *browptr,
                     const int32_t *bcol, const double *blocks_ri, mgcr_op_t *out);
int mgcr_op_destroy(mgcr_op_t op);
int64_t mgcr_op_dim(mgcr_op_t op);                                 /* get_dim src/Operator.h:21 */
int64_t mgcr_op_nrow(mgcr_op_t op);
int64_t mgcr_op_nnz(mgcr_op_t op);
/* y = op(x)        Operator::operator() src/Operator.h:19; Sparse :330-346; DiracOp :569-575;
 *                  HierarchicalSparse.h:101-161; GCR.h:62-68; MG.h:124-129 */
int mgcr_op_apply(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y);
/* Y = op(X) for a block of k Fields: the matrix is read once for all k columns.  Column j of Y is BIT-IDENTICAL to
 * mgcr_op_apply on column j: per column the kernels add a row's products in the order mgcr_op_ell_layout documents (block-CSR:
 * per block in column order, blocks in storage order), whichever storage form carries the matrix.  Supported: single-GPU
 * Sparse in every storage form (ELL slab + CSR tail with 1 .. 16 lanes per row, the LDS-window variant, both row-pattern
 * dictionary forms, the stencil view), DiracOp and MultiDiracOp on top of any of them, MultiEvenOddDiracOp (blocks of its even half), HierarchicalSparse / Dense.  Distributed operators
 * and GCR / MG objects: MGCR_ERR_UNSUPPORTED.  X == Y, mismatched n or k: MGCR_ERR_INVALID.
 * Block-CSR stages min(k, 64 / bs) (at least 1) columns of products and k columns of accumulators in LDS,
 * 16 (kg bs (bs + 1) + bs k) bytes: block sizes for which that exceeds 160 KiB (bs from about 95, depending on k) are
 * MGCR_ERR_UNSUPPORTED here although the single apply takes them up to bs = 100. */
int mgcr_op_apply_multi(mgcr_op_t op, mgcr_mvec_t x, mgcr_mvec_t y);
/* bytes the device layout of `op` occupies / streams per apply (for roofline accounting) */
int mgcr_op_stored_bytes(mgcr_op_t op, int64_t *matrix_bytes, int32_t *ell_width, int64_t *tail_nnz);
/* storage a Sparse ended up with: *format = 0 plain ELL slab (+ CSR tail), 1 row-pattern dictionary
 * holding column offsets and values, 2 row-pattern dictionary for the columns + value slab;
 * *n_patterns = dictionary size (0 for format 0) */
int mgcr_op_storage_format(mgcr_op_t op, int32_t *format, int32_t *n_patterns);
/* how the rows of a Sparse are dealt to threads — what decides the order in which a row's products are added, i.e. the
 * one thing in which y = A x may differ from the reference's row loop (src/Operator.h:338-341): *ell_width = W, entries
 * 0..W-1 of a row sit in the ELL slab; *lanes = L, lane l of L adds entries l, l+L, ... in order and the L sums are
 * combined by a tree (L = 1: CSR order, bit-identical to the reference); *tail_rows = rows longer than W: their remaining
 * entries are summed in CSR order by one thread (products staged in LDS) and added to the row's ELL sum — unless there are
 * more than *tail_chunk_cap of them, which one wave sums (64 lanes striding, tree); *reach = max |column - row| when the
 * operator has a row-pattern dictionary, else 0 (it decides the row -> workgroup map of the GCR kernels that embed the
 * apply); *x_window = H > 0 when the stand-alone apply stages x[tile - H, tile + 1024 + H) in LDS (banded irregular matrices:
 * >= 90 % of the slab's columns within H rows of their row; no influence on the bits).  Any pointer may be NULL.  tests/test_gpu_bitwise.py feeds these to the CPU oracle's model of the device's
 * summation order. */
int mgcr_op_ell_layout(mgcr_op_t op, int32_t *ell_width, int32_t *lanes, int64_t *tail_rows, int64_t *reach, int32_t *tail_chunk_cap,
                       int32_t *x_window);
/* Where a lean restarted GCR on this operator forms r' = r - alpha A p: *kind = 0 in a launch of its own (xr_update_kernel), 1 inside
 * the kernel that embeds the apply, latency regime (same sums, same bits), 2 inside the windowed apply of the bandwidth regime
 * (csrc/gcr_fused_xr_tile.h: |r'|^2 is then summed over that kernel's banded row map — tests/test_gpu_bitwise.py tells the oracle). */
int mgcr_op_xr_fuse_kind(mgcr_op_t op, int32_t *kind);
/* Sparse::dagger / mod_*_at (src/Operator.h:296-328,84-86) change a Sparse IN PLACE while a DiracOp, GCR or MG may hold a
 * pointer to it (src/Operator.h:117): this replaces the matrix behind an existing handle, so that every operator that
 * borrowed the handle (mgcr_dirac_create, mgcr_gcr_create) applies the new matrix.  On failure the old matrix stays.
 * Not for the row block of a distributed Sparse.  (An MG hierarchy built from the old matrix is not rebuilt — nor is the
 * reference's, src/MG.h:131-285.) */
int mgcr_csr_replace(mgcr_op_t op, int64_t nrow, int64_t ncol, const int64_t *rowptr, const int64_t *col, const double *val_ri);
/* Implementation switches (default on unless noted; each also has an environment variable read at first use).
 * They select between code paths that compute the same thing; tests use them to compare the paths.
 *   "pattern_storage" ($MGCR_PATTERNS): try the row-pattern dictionary for every Sparse of >= 2^15 rows
 *                      created while it is on;
 *   "lean_cycles"     ($MGCR_LEAN): restart-mode GCR keeps residuals instead of search directions inside
 *                      a restart cycle (same r, Ap and scalars; x differs by rounding);
 *   "fused_apply"     ($MGCR_FUSE): GCR on a Sparse / DiracOp runs the SpMV and the beta dot
 *                      products of its result as one kernel (same bits as the two kernels);
 *   "graph_replay"    ($MGCR_GRAPH, default OFF): restart cycles of systems of <= 2^18 rows are captured in a
 *                      hipGraph once and replayed (same kernels, same results; measured slower than eager
 *                      launches since the iteration shrank to 3 kernels, see gcr.hip).
 *   "resident_solver" ($MGCR_RESIDENT): a lean restarted GCR solve on a stencil-view Sparse / DiracOp of at most one row per
 *                      thread of the chip (<= 262 144 rows) runs as ONE launch with its vectors in registers
 *                      (csrc/gcr_resident.hip; same iterates, bit for bit, as the multi-kernel path).
 *   "step_build"      ($MGCR_STEPBUILD): a lean step with up to 5 stored directions on a 7-point stencil-view operator of 2^19 .. 2^21
 *                      rows runs its apply, dot products and direction build as one launch, A r staying in LDS
 *                      (csrc/gcr_stepbuild.hip; same iterates, bit for bit, as the two kernels).
 *   "halo_split"      ($MGCR_HALO_SPLIT): the stand-alone apply of a distributed Sparse whose halo travels by peer writes stores and
 *                      publishes its boundary rows, multiplies the rows that need no halo, THEN waits for the neighbours and
 *                      multiplies the boundary rows (same bits; off: the exchange completes before any row).
 *   "pw_tail"         ($MGCR_PW_TAIL): on a distributed operator whose scalars travel by peer writes, the kernel that produces a
 *                      reduction's partials (apply + dot products of a stencil row block; direction build up to 8 directions) also
 *                      folds them and sums them over the ranks in its last workgroup — no fold + exchange launch behind it (same bits).
 *   "spmv_part"       (measurement aid, default 0): 1 = a Sparse apply launches only its ELL-slab kernel, 2 = only its CSR-tail
 *                      kernel (bench.py times the two parts of the hybrid layout separately); 0 = the whole apply.
 * *previous (may be NULL) receives the old value. */
int mgcr_set_option(const char *name, int value, int *previous);
/* Counters for tests and benchmarks: "resident_solves" = GCR solves that took the one-launch path since mgcr_init,
 * "step_build_launches" = steps that ran as one apply + build launch, "small_solves" = solves that ran as one launch of one
 * workgroup (csrc/gcr_small.hip), "one_launch_fallbacks" = top-level solves that were repeated on the multi-kernel path
 * because a one-launch path gave up (foreign work on the device: its grid was not co-resident), "halo_split_exchanges" =
 * peer-write halo exchanges of distributed applies that ran split (store + publish | interior rows | wait | boundary rows),
 * "pw_tail_folds" = reductions folded and summed over the ranks inside their producing kernel, "multi_solves" = batched solves
 * (mgcr_gcr_solve_multi) completed — queued solves are not counted there but in "queue_solves" = mgcr_gcr_solve_queue calls completed,
 * "queue_admissions" = systems those loaded into a slot after step 0, "queue_steps" = lockstep steps they launched,
 * "eo_queue_solves" / "eo_queue_admissions" / "eo_queue_steps" = the same three for mgcr_eo_solve_queue,
 * "evenodd_fused_steps" = GCR steps on an even-odd preconditioned DiracOp whose second apply stage took the step's beta dot
 * products (mgcr_eo_create, Rule 2),
 * "evenodd_diag_fused_steps" = the same on an operator that carries a site diagonal (mgcr_eo_create_diag, Rule 2d),
 * "evenodd_block_applies" = Schur applies of an operator with a dense block per site (mgcr_eo_create_block), inside GCR steps or
 * not, "evenodd_block_fused_steps" = its GCR steps whose last apply launch took the step's beta dot products (Rule 3b),
 * "gcr32_applies" = applies of a low-precision GCR (mgcr_gcr32_create) that ran on the device, "gcr32_steps" = the inner steps those
 * enqueued (both kept on the device: one synchronisation per query), "gcr32_multi_applies" = batched applies of a low-precision
 * GCR (mgcr_gcr32_apply_multi, mgcr_gcr32_solve_multi) enqueued, "gcr32_multi_steps" = the lockstep steps those enqueued,
 * "multi_flex_solves" = flexible batched solves (mgcr_gcr_solve_multi with a right preconditioner) completed — "multi_solves" counts
 * them as well, and the batched applies they enqueue move "gcr32_multi_applies" and "gcr32_multi_steps". */
int mgcr_stat(const char *name, int64_t *value);

/* Self-test of the hardware behaviour the one-launch solver paths (csrc/gcr_resident.hip, gcr_stepbuild.hip) build on: inside
 * ONE launch, rows stored with `buffer_store ... sc1` by one workgroup are read correctly with `buffer_load ... sc1` by
 * workgroups of other XCDs after a fence-free {value, generation} exchange.  Runs `steps` dependent steps over one
 * workgroup per CU with the library's own primitives and bounded polls; *rows_wrong = entries that differ from what the
 * host computes (0 expected).  coherent = 0 runs the control with ordinary loads / stores (expected to FAIL: it shows the
 * test can).  tests/test_gpu_resident.py runs both on every GPU test pass. */
int mgcr_selftest_coherence(int32_t steps, int32_t coherent, int64_t *rows_wrong);

/* ---- GCR: src/GCR.h, src/SolverParam.h ---------------------------------------------------- */
typedef struct mgcr_gcr_param {
    /* GCR_Param (src/SolverParam.h:21-35) */
    int32_t truncation; /* != 0: ring of `truncation` directions, never wiped      */
    int32_t restart;    /* != 0: `restart` slots, all wiped every `restart` steps  */
    int32_t max_iter;   /* do..while: at least one iteration even for 0 (src/GCR.h:222,288) */
    double tol;         /* stop when |r|^2/|b|^2 <= tol^2 (src/GCR.h:288)          */
    int32_t verbose;    /* print "Step %d residual norm = %.10e" lines (src/GCR.h:214,271) */
    mgcr_op_t left_precond;  /* SolverParam (src/SolverParam.h:10-18); may be NULL */
    mgcr_op_t right_precond;
    /* extensions, 0 = the reference's behaviour */
    int32_t use_x0;      /* 1: r0 = b - A x0 (the reference uses r0 = b, src/GCR.h:189) */
    int32_t flexible;    /* 1: flexible right preconditioning (p = M r, true residual kept)
                            instead of the reference's literal r = M(r) (src/GCR.h:236-238) */
    int32_t check_every; /* host looks at the device-side convergence flag every this many
                            iterations (0 = library default); results do not depend on it */
    int32_t profile_spmv; /* 1: bracket the phases of every iteration with hipEvents on the library
                            stream; read the result with mgcr_gcr_last_profile (bench.py) */
} mgcr_gcr_param;

/* GCR::solve(rhs, x) (src/GCR.h:158-302).  hist[0] is the step-0 entry, hist[k] the value
 * printed at step k (sqrt(|r|^2)/|b|); at most hist_cap entries are written (hist may be NULL).
 * *n_iter = iterations performed (global_count); *converged = 0 iff n_iter == max_iter. */
int mgcr_gcr_solve(mgcr_op_t A, const mgcr_gcr_param *param, mgcr_vec_t rhs, mgcr_vec_t x,
                   double *hist, int32_t hist_cap, int32_t *n_iter, int32_t *converged);
/* The even-odd preconditioned solve of (1 - k D) x_full = b_full: see mgcr_eo_create. */
int mgcr_eo_solve(mgcr_op_t eo, const mgcr_gcr_param *param, mgcr_vec_t b_full, mgcr_vec_t x_full,
                  double *hist, int32_t hist_cap, int32_t *n_iter, int32_t *converged);
/* The batched even-odd preconditioned solves of (1 - k_j D) x_full,j = b_full,j: see mgcr_eo_multi_create. */
int mgcr_eo_multi_solve(mgcr_op_t op, const mgcr_gcr_param *param, mgcr_mvec_t B_full, mgcr_mvec_t X_full,
                        double *hist /* [nk][hist_cap] */, int32_t hist_cap, int32_t *n_iter, int32_t *converged);
/* k independent solves A x_j = rhs_j that share every launch (batched restarted GCR, csrc/gcr_multi.hip).
 * hist: [k][hist_cap] (may be NULL), row j as mgcr_gcr_solve fills it for column j; n_iter, converged: [k] (may be NULL).
 * Every column has its own device-resident scalars and stop flag; a column that has stopped (|r|^2/|b|^2 <= tol^2, or
 * whatever stops the single solve) is FROZEN — its x, residual, history and iteration count no longer change — while the
 * others go on; the solve ends when every column has stopped or at max_iter.  x is updated in place; use_x0 as in
 * mgcr_gcr_solve.
 * Supported: restart mode (restart != 0, cycles of at most 16 steps), unpreconditioned — or with a flexible right preconditioner,
 * see "Flexible batched GCR" below —, on the operators of
 * mgcr_op_apply_multi.  MGCR_ERR_UNSUPPORTED: truncation != 0, restart == 0, restart > 16 (with max_iter >= 16), a left or
 * right preconditioner, flexible (other than the flexible right preconditioners of the block below), profile_spmv, distributed
 * operators, GCR / MG objects as the operator.
 * Arithmetic: the lean restart cycle of mgcr_gcr_solve per column, with the same rows per thread, grid size, summation trees
 * and folds: history, iteration count, convergence flag and x of column j are BIT-IDENTICAL to mgcr_gcr_solve(A, param, rhs_j)
 * with default options, for operators whose mgcr_op_xr_fuse_kind is 0 or 1 and more rows than the small-solve limit
 * (mgcr_set_small_solve_rows).  Where the single solve sums in another order — the one-workgroup path at or below that limit,
 * and mgcr_op_xr_fuse_kind == 2 (grids from 182^3: |r'|^2 and the start-up sums run over a banded row map) — the batched solve
 * sums in the plain row order and the results agree to rounding only.  There is no one-workgroup batched form.
 * The work vectors (2 + 2 * min(restart, max_iter + 1) blocks of n x k) are kept by the library from one batched solve to the
 * next while n, k and the cycle length stay the same, and are freed by mgcr_finalize.
 *
 * Flexible batched GCR: mgcr_gcr_solve_multi with param->flexible == 1 and param->right_precond = M (csrc/gcr_multi.hip, the device
 * side csrc/gcr_multi_flex.hip).  Slot kinds:
 *   (a) a LowPrecisionGCR of the square form (mgcr_gcr32_create, Dirac or matrix form) with n equal to the block's rows: it runs as
 *       the k-wide LOCKSTEP inner solve of mgcr_gcr32_apply_multi, the fp32 slab streamed once per inner step for all k columns.  The
 *       preconditioner keeps its own k32 — a preconditioner at another k is legitimate, so a MultiDiracOp as A is accepted;
 *   (b) any operator that mgcr_op_apply_multi takes on one GPU with dim n and n rows (Sparse, DiracOp, HierarchicalSparse), applied
 *       k-wide to the residual block.
 * A: whatever mgcr_gcr_solve_multi takes unpreconditioned on n rows, a MultiDiracOp included.
 * Per column the recurrences are the single solve's lean flexible cycle: r0 = b (use_x0: b - A x0), Z = M r0 with every column
 * taking part, P0 = Z, Ap0 = A P0; per step alpha, r -= alpha Ap IN PLACE (the residual ring is not written), D = M r into the slot
 * of the next direction — into a block of its own on the step that closes a cycle —, A D, the beta dots, the build; there is no
 * preconditioner behind a solve's last update.
 * Rule F: history, iteration count, convergence flag and x of column j are BIT-IDENTICAL to mgcr_gcr_solve(A_j, param, rhs_j) with
 * the same preconditioner in the slot, on column j alone (A_j = DiracOp(D, ks[j]) for a MultiDiracOp) — for every k, every column
 * position and whatever the other columns do; default options, mgcr_op_xr_fuse_kind 0 or 1.  The small-solve limit does not enter:
 * a single solve with any preconditioner never takes the one-workgroup path (gcr_small_eligible returns false for a left or right
 * preconditioner and for profile_spmv) nor the resident one-launch path, so Rule F holds at every n.
 * The mask: a column that has stopped is FROZEN with x updates still pending in the slots; the preconditioner stores D to the
 * columns that are still active at the step only — a frozen column's slots keep their bits until the pending updates are applied.
 * The gate: behind the inner solve's entry, one launch per outer step evaluates per column the outer solve's own stopping test
 * (the fold of the step's |r|^2 partials, |b|^2, tol^2: the solver's fold and expression, the bits of the single solve's gate) and
 * cuts the inner solve of a column that is frozen, or about to end on this residual, to 0 steps; a gated column that is still
 * active gets D = 0, as in the single solve.  mgcr_gcr32_last_multi then reports 0 steps for it.  Kind (b) is not gated.
 * Launches per outer step, whatever the data: the unpreconditioned step's, plus for (a) the batched apply's
 * 4 m + 2 - ceil(m / restart_inner) (m = the inner max_iter) plus 1, the gate; for (b) the k-wide apply of M plus, off the closing
 * step, 1 masked copy.  No host round trip is added: the host polls every check_every steps as before.  The unpreconditioned
 * solve enqueues exactly the launches it enqueued before.
 * Storage: one more n x k block (3 + 2 * min(restart, max_iter + 1) in all), allocated only by a flexible solve; storage made by a
 * flexible solve serves an unpreconditioned one at the same n, k and cycle length, not the reverse.  (a) also uses the operator's own
 * k-wide storage (mgcr_gcr32_apply_multi).
 * Counters (mgcr_stat): "multi_flex_solves" = flexible batched solves completed ("multi_solves" counts them too);
 * "gcr32_multi_applies" and "gcr32_multi_steps" count the applies and lockstep steps these solves enqueue.
 * MGCR_ERR_UNSUPPORTED: a left preconditioner; a right preconditioner with flexible == 0; flexible == 1 without one; a GCR or MG object
 * in either slot; an even-odd `low` (mgcr_gcr32_create_eo); a MultiDiracOp or MultiEvenOddDiracOp in the slot; an even-odd
 * preconditioned DiracOp in the slot; a low-precision GCR as A; profile_spmv, distributed operators (A or M), truncation or full
 * mode, cycles longer than 16.  MGCR_ERR_INVALID: a preconditioner whose dimension is not n or that is not square.  Nothing is
 * written to x in any refused call.  mgcr_eo_multi_solve, mgcr_gcr_solve_queue and mgcr_eo_solve_queue go on refusing every
 * preconditioner. */
int mgcr_gcr_solve_multi(mgcr_op_t A, const mgcr_gcr_param *param, mgcr_mvec_t rhs, mgcr_mvec_t x, double *hist, int32_t hist_cap,
                         int32_t *n_iter, int32_t *converged);
/* Queued batched GCR: nsys independent systems (any nsys) stream through `width` <= 16 slots (columns) of ONE batched restarted solve
 * (csrc/gcr_multi.hip; the schedule is csrc/queue_plan.h).  System s: A x_s = rhs_s (k_ri == NULL), or (1 - k_s D) x_s = rhs_s with
 * A = D a single-GPU Sparse (k_ri: [nsys][2], no zero entry).  At step 0 the first min(width, nsys) systems occupy the slots; a slot
 * whose system has stopped is drained (its x, history, iteration count handed back) and refilled with the next waiting system, first
 * in, first out, at the next boundary of the restart cycle — or at once when every slot has stopped.  The host drives all of it
 * between launches: it polls the columns' device states at every cycle boundary and every check_every steps; no kernel waits on
 * another.  width > nsys is allowed (the surplus slots stay empty).
 * rhs, x: [nsys] Fields of the operator's dimension.  rhs handles may repeat (a scan has one b); the x handles must be pairwise
 * distinct and none of them may be a right-hand side (MGCR_ERR_INVALID, nothing is touched).  x_s is read and updated in place as
 * mgcr_gcr_solve does it, use_x0 included.  hist: [nsys][hist_cap] or NULL; n_iter, converged: [nsys] or NULL — per SYSTEM, in
 * the caller's order.
 * Operators: k_ri == NULL — whatever mgcr_gcr_solve_multi takes except a MultiDiracOp (its width is a block's:
 * MGCR_ERR_UNSUPPORTED); k_ri != NULL — a plain single-GPU Sparse (MGCR_ERR_INVALID otherwise, MGCR_ERR_UNSUPPORTED when it is
 * distributed).  MGCR_ERR_UNSUPPORTED: every case of mgcr_gcr_solve_multi (truncation != 0, restart == 0, cycles longer than 16, a
 * preconditioner, flexible, profile_spmv, distributed operators, GCR / MG objects).  MGCR_ERR_INVALID: width outside 1 .. 16,
 * nsys < 1, a null handle, a size mismatch.
 * Rule: history, iteration count, convergence flag and x of system s are BIT-IDENTICAL to mgcr_gcr_solve on that system alone (with
 * k_ri: on DiracOp(D, k_s)), under the conditions mgcr_gcr_solve_multi states (default options, mgcr_op_xr_fuse_kind 0 or 1, more
 * rows than the small-solve limit) — whatever the width, the order of the systems and check_every.
 * The work storage is mgcr_gcr_solve_multi's at k = min(width, nsys) plus two blocks (x, b), kept and freed likewise. */
int mgcr_gcr_solve_queue(mgcr_op_t A, const mgcr_gcr_param *param, int32_t width, int32_t nsys, const mgcr_vec_t *rhs, const mgcr_vec_t *x,
                         const double *k_ri, double *hist, int32_t hist_cap, int32_t *n_iter, int32_t *converged);
/* Queued even-odd scan: nsys systems (1 - k_s D) x_s = rhs_s on FULL Fields of n entries (any nsys) stream through
 * W = min(width, nsys) columns of ONE batched solve of the Schur systems S_s = 1 - k_s^2 D_eo D_oe on blocks of n_e rows
 * (csrc/evenodd_queue.hip on the driver of mgcr_gcr_solve_queue; the schedule is csrc/queue_plan.h unchanged).  eo is an even-odd
 * preconditioned DiracOp (mgcr_eo_create): its halves and index lists are borrowed, its own k is neither used nor changed.
 * k_ri: [nsys][2], no zero entry.  Admitting system s into slot j forms bhat_e = b_e + k_s D_eo b_o into column j, takes the even
 * half of x_s as the column's x (the start vector under use_x0, exactly as in mgcr_eo_solve) and keeps b_o in column j of an
 * [n_o x W] block while the system is in flight; retiring slot j applies the column's pending x updates, forms
 * x_o = b_o + k_s D_oe x_e and writes both halves into x_s.  An admission point costs a fixed number of passes, one k-wide shifted
 * D_eo apply and the queue's one (use_x0: two) k-wide Schur applies, a retirement point one k-wide shifted D_oe apply, whatever
 * the number of columns admitted or retired.  The host drives everything between launches; no kernel waits on another.
 * rhs handles may repeat; the x handles must be pairwise distinct and none may be a right-hand side.  hist: [nsys][hist_cap] or
 * NULL, row s relative to |bhat_e,s|; n_iter, converged: [nsys] or NULL — per SYSTEM, in the caller's order.
 * MGCR_ERR_INVALID (nothing is enqueued or touched): eo is not an EvenOddDiracOp (a MultiEvenOddDiracOp, a Sparse, a DiracOp),
 * k_ri == NULL, a zero k_s, width outside 1 .. 16, nsys < 1, a null handle, a Field whose length is not n (a Field of n_e
 * entries is the likely slip), an x that repeats or is a right-hand side.  MGCR_ERR_UNSUPPORTED: every parameter case of
 * mgcr_eo_multi_solve (truncation != 0, restart == 0, cycles longer than 16, a preconditioner, flexible, profile_spmv).
 * Rule: history, iteration count, convergence flag and the whole x_full of system s are BIT-IDENTICAL to mgcr_eo_solve on
 * EvenOddDiracOp(D, k_s) with that system alone — at any size, width, order of the systems and check_every, and on every storage
 * form of the halves (Rules 1 and 2 of mgcr_eo_multi_create and the rule of mgcr_gcr_solve_queue; a Schur solve never takes a
 * one-workgroup or one-launch path, so the small-size exception does not arise).
 * Counters (mgcr_stat): "eo_queue_solves" = calls completed, "eo_queue_admissions" = systems loaded into a slot after step 0,
 * "eo_queue_steps" = lockstep steps launched; "queue_*" and "multi_solves" do not move.
 * The work storage is mgcr_gcr_solve_queue's at k = W on n_e rows, plus the slot operator's blocks (b_e, b_o, bhat, x_e, x_o, the
 * D_oe product between the two stages; one more per half with a CSR tail), kept by the library between calls while n_e, n_o and
 * W stay the same and freed by mgcr_finalize.  mgcr_gcr_solve_queue itself goes on refusing both even-odd kinds. */
int mgcr_eo_solve_queue(mgcr_op_t eo, const mgcr_gcr_param *param, int32_t width, int32_t nsys, const mgcr_vec_t *rhs_full,
                        const mgcr_vec_t *x_full, const double *k_ri /* [nsys][2] */, double *hist /* [nsys][hist_cap] or NULL */,
                        int32_t hist_cap, int32_t *n_iter, int32_t *converged);
/* Unpreconditioned solves on a single-GPU Sparse / DiracOp with at most `rows` unknowns (default
 * 1024, $MGCR_SMALL_SOLVE_ROWS; and at most 16*rows stored entries) and <= 8 stored directions run
 * as ONE launch of one workgroup (latency regime: coarsest multigrid levels); 0 disables that path.
 * Same arithmetic, dot products summed in a different fixed order. */
int mgcr_set_small_solve_rows(int64_t rows);
/* GCR as an Operator (src/GCR.h:19-50,62-68): apply(f) solves A x = f.  A may be NULL and be
 * supplied later with mgcr_gcr_set_operator (GCR(GCR_Param*) + initialise(), src/GCR.h:30-31).
 * x0_mode 0: x0 = the vector given with mgcr_gcr_set_x0 (the reference seeds x0 with
 * init_rand(2)); 1: x0 = 0.  Used as smoother / coarse solver / preconditioner, it runs without
 * host round-trips: the device-side convergence flag turns the remaining iterations into no-ops. */
int mgcr_gcr_create(mgcr_op_t A, const mgcr_gcr_param *param, int32_t x0_mode, mgcr_op_t *out);
int mgcr_gcr_set_operator(mgcr_op_t gcr, mgcr_op_t A);
/* GCR::solve(rhs, x) on a GCR object made with mgcr_gcr_create: same as mgcr_gcr_solve, but the
 * work vectors (r, Ar, the direction slots, reduction slabs) live in the object and are re-used
 * from solve to solve instead of being allocated and freed around every call.  The reference's GCR
 * reads its GCR_Param* at solve time (src/GCR.h:171-185); mgcr_gcr_set_param is that refresh. */
int mgcr_gcr_set_param(mgcr_op_t gcr, const mgcr_gcr_param *param);
int mgcr_gcr_solve_op(mgcr_op_t gcr, mgcr_vec_t rhs, mgcr_vec_t x, double *hist, int32_t hist_cap,
                      int32_t *n_iter, int32_t *converged);
int mgcr_gcr_set_x0(mgcr_op_t gcr, mgcr_vec_t x0);

/* LowPrecisionGCR: mixed precision (new — every other object of the library is complex fp64).  The operator owns an fp32 copy of a
 * matrix; applied to an fp64 Field f (mgcr_op_apply) it returns y ~ A^-1 f from a restarted GCR that runs entirely in fp32 on the
 * device, from x0 = 0, with no host round trip (csrc/gcr32.hip).  Its place is the right_precond slot of an fp64 solve with
 * flexible = 1: the cheap inexact inner solve does most of the work, the fp64 outer GCR keeps the true residual.
 * The host CSR (int64 indices) is copied like mgcr_eo_create's.  k_ri != NULL: Dirac form, A = 1 - k D; k_ri == NULL: matrix form,
 * A = the matrix.  `inner` reads restart (1 .. 16 slots), max_iter (>= 1: the steps enqueued per apply, 3 launches each, plus an
 * entry and an exit launch) and tol (relative: the solve stops when |r|^2 <= tol^2 |f|^2; a tol below fp32's reach is accepted
 * and simply runs max_iter steps).
 * Arithmetic.  fp32 complex is float2.  A value is (float)re, (float)im, round to nearest; k32 = (float)k.  Products are
 * (ar br - ai bi, ar bi + ai br) in float, nothing is fused.  Row sum: the first W entries of a row (the ELL part, W from
 * mgcr_gcr32_info, the plain Sparse slab's pick) are added in stored order into an accumulator that starts at +0; a row's remaining
 * entries (the tail) are added in stored order into a second accumulator, which is then added to the first.  When every stored
 * imaginary part is zero the slab is real (4 B per value) and a product is (a br, a bi).  Dirac form: y = x - k32 s.  Dot products
 * and norms: every fp32 operand is converted to double, products and sums are fp64, per-workgroup partial slabs folded by the
 * consumer in a fixed order (csrc/reduce.h) — no atomics, an apply is bit-reproducible run to run.  Scalars: alpha and the beta_j are
 * formed in fp64 from the fp64 sums (a complex sum divided by a real one, component by component) and rounded to float once.  The
 * iteration is the classic restarted GCR: r = fp32(f), x = 0; per step p = r, Ap = A r; beta_j = <Ap_j, Ap> / <Ap_j, Ap_j> and
 * p -= beta_j p_j, Ap -= beta_j Ap_j over the stored directions in slot order (<a, b> = sum conj(a) b); alpha = <Ap, r> / <Ap, Ap>;
 * x += alpha p, r -= alpha Ap; all slots are wiped every `restart` steps.  The tolerance is tested at the start of a step, on the
 * |r|^2 the step before left and |f|^2 = |fp32(f)|^2.  f = 0, or an exactly zero <Ap, Ap>, stops the solve with what x holds: f = 0
 * gives y = 0, never NaN.  y = fp64(x).
 * MGCR_ERR_UNSUPPORTED, with a message: truncation != 0, restart == 0 or restart > 16, any preconditioner, use_x0, flexible or
 * profile_spmv in `inner`.  MGCR_ERR_INVALID: max_iter < 1, a negative tol, a non-square matrix (a column outside 0 .. n-1) or
 * inconsistent CSR, k = 0, mgcr_gcr32_set_k on the matrix form, a stored value or a k that is not finite or becomes infinite when
 * rounded to float (the message names the row).  A refused mgcr_gcr32_set_k / mgcr_gcr32_set_param leaves the operator as it was.
 * Accepted by mgcr_op_apply (fp64 Fields of n entries), mgcr_op_destroy, mgcr_op_dim / nrow / nnz, and by the right_precond slot of
 * mgcr_gcr_solve, mgcr_gcr_create (+ mgcr_gcr_set_param) and mgcr_gcr_solve_op — but only with flexible = 1: the inner solve stops
 * on a tolerance, so it is not a linear map.  With flexible = 0, or in the left_precond slot: MGCR_ERR_UNSUPPORTED; a dimension that
 * differs from the outer operator's: MGCR_ERR_INVALID; a distributed outer operator: MGCR_ERR_UNSUPPORTED.
 * Refused with MGCR_ERR_UNSUPPORTED: as the system operator of any solve (mgcr_gcr_solve, mgcr_gcr_create, mgcr_gcr_set_operator),
 * mgcr_mg_create, mgcr_op_apply_multi, mgcr_gcr_solve_multi, mgcr_gcr_solve_queue, mgcr_eo_solve_queue and the storage queries
 * (mgcr_op_stored_bytes / storage_format / ell_layout / xr_fuse_kind / halo_kind; ask mgcr_gcr32_info).  mgcr_gcr_solve_multi refuses
 * it as its operator A; the right_precond slot of that solve, flexible = 1, takes it (the "Flexible batched GCR" block there).
 * All storage (r, Ar, x, 2 * restart slots, slabs, state) belongs to the operator: allocated here or by mgcr_gcr32_set_param, freed by
 * mgcr_op_destroy.  k travels in the kernel arguments of every launch: what is already enqueued keeps the old value.
 * In the right_precond slot the apply that follows an outer step's residual update is handed that solve's own stopping test (the
 * |r|^2 partials, |b|^2, tol^2) and evaluates it with the solver's fold and expression: behind the LAST update — the outer solver
 * enqueues its preconditioner before the step's test — the inner solve is cut to 0 steps and y = 0, which nothing reads.
 * Counters (mgcr_stat, one synchronisation each): "gcr32_applies" = applies that ran on the device, "gcr32_steps" = the inner steps
 * those enqueued (max_iter per apply); an apply silenced because its outer solve was over, or cut as above, counts in neither: a
 * mixed solve of N outer steps moves them by N and max_iter N. */
int mgcr_gcr32_create(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri, const double *k_ri,
                      const mgcr_gcr_param *inner, mgcr_op_t *out);
int mgcr_gcr32_set_k(mgcr_op_t op, const double k_ri[2]);          /* Dirac form only */
int mgcr_gcr32_set_param(mgcr_op_t op, const mgcr_gcr_param *inner);
/* stored_bytes: the fp32 matrix copy (slab, tail, their index tables) */
int mgcr_gcr32_info(mgcr_op_t op, int64_t *n, int32_t *ell_width, int64_t *tail_rows, int32_t *real_slab, int64_t *stored_bytes);
/* test hook: y = fp64(A32 fp32(x)), one matrix apply in fp32 (BIT-IDENTICAL to the arithmetic above; uses the operator's r and Ar) */
int mgcr_gcr32_apply_matrix(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y);
/* ONE synchronisation: steps the last apply performed and its last fp32 |r| / |f| */
int mgcr_gcr32_last(mgcr_op_t op, int32_t *n_iter, double *rel_res);

/* LowPrecisionEvenOddGCR: the low-precision GCR on the EVEN-ODD Schur system (csrc/gcr32_eo.hip).  The operator is an OP_GCR32 like
 * the one above, with dim = nrow = n_e, whose matrix is the fp32 copy of
 *     S = diag(a_e) - c^2 H_eo diag(1 / a_o) H_oe
 * for the scalar forms of the even-odd operators: k_ri != NULL, Dirac form (a = 1 - k d, c = k; a matrix without a stored diagonal
 * entry is the pure hopping operator of mgcr_eo_create and stores no a); k_ri == NULL, matrix form (a = d, c = -1).  Dense site
 * blocks (mgcr_eo_create_block) are not covered.  Its place is the right_precond slot, flexible = 1, of mgcr_eo_solve, of
 * mgcr_gcr_solve on an even-odd operator and of a GCR object; the inner GCR, its parameters, counters, mgcr_gcr32_set_k (Dirac form
 * only), mgcr_gcr32_set_param, mgcr_gcr32_last and mgcr_gcr32_apply_matrix (Fields of n_e entries) are those of mgcr_gcr32_create;
 * mgcr_op_nnz returns that of the stored matrix; mgcr_gcr32_info returns MGCR_ERR_UNSUPPORTED (ask mgcr_gcr32_eo_info).
 * Colouring and refusals are mgcr_eo_create_diag's: the same host plan, the same message for a conflicting entry, k = 0 and a 1 / a_o
 * that is exactly zero or not finite are MGCR_ERR_INVALID (the message names the full-system row); and so is a stored value, an a, a
 * 1 / a_o, a k or a c^2 that is not finite in float.  A refused mgcr_gcr32_set_k leaves the operator as it was.
 * Arithmetic (everything not said here is mgcr_gcr32_create's).  a and 1 / a_o are formed in fp64 by the operations
 * mgcr_eo_create_diag documents (Rule 1d) and then rounded, (float)re, (float)im: mgcr_gcr32_eo_diag returns float32 of what
 * mgcr_eo_diag returns for the same matrix and k, bit for bit.  c2_32 = (float) of c c, the product formed un-fused in fp64.  An
 * off-diagonal value is (float)re, (float)im; the slabs are real when every stored off-diagonal imaginary part is zero — one flag
 * for both halves.  Each half has the layout of the square form (its own W, slab [W][npad], tail with its own accumulator), and a
 * row of either half is summed exactly as a row of the square form.
 *   stage 1, odd rows:    u = H_oe32 r;  t = inv_o32 (.) u, an un-fused complex product  (t = u when no diagonal is stored)
 *   stage 2, even rows:   v = H_eo32 t;  w = c2_32 v (un-fused);  y = a_e32 (.) r - w    (y = r - w when no diagonal is stored)
 * 4 launches per inner step, 4 max_iter + 2 per apply.  The operator owns t (n_o elements).  a_e32 and inv_o32 are rewritten by
 * mgcr_gcr32_set_k in stream order (what is enqueued keeps the old values), c2_32 travels in the kernel arguments.
 * Slot check, in addition to mgcr_gcr32_create's: when the operator of the solve is itself an even-odd operator of the scalar forms,
 * its n and its parity vector must equal this operator's (MGCR_ERR_INVALID: another colouring would still converge, slowly and
 * silently); when it carries site blocks: MGCR_ERR_UNSUPPORTED.  k is NOT compared — a preconditioner at another k is legitimate.
 * The batched and queued solves refuse any preconditioner of this even-odd form: mgcr_eo_multi_solve and the queues take none at
 * all, mgcr_gcr_solve_multi the square form of mgcr_gcr32_create only (its "Flexible batched GCR" block). */
int mgcr_gcr32_create_eo(int64_t n, const int64_t *rowptr, const int64_t *col, const double *val_ri,
                         const int8_t *parity /* NULL: two-colour */, const double *k_ri /* NULL: matrix form */,
                         const mgcr_gcr_param *inner, mgcr_op_t *out);
/* widths and tail rows of H_eo and H_oe; stored_bytes: both fp32 halves and, when stored, a_e and 1 / a_o */
int mgcr_gcr32_eo_info(mgcr_op_t op, int64_t *n, int64_t *n_even, int64_t *n_odd, int32_t *width_eo, int32_t *width_oe,
                       int64_t *tail_rows_eo, int64_t *tail_rows_oe, int32_t *real_slab, int32_t *has_diag, int64_t *stored_bytes);
/* a_e32 and inv_o32 as the device holds them ((1, 0) when no diagonal is stored) */
int mgcr_gcr32_eo_diag(mgcr_op_t op, float *a_even_ri /* [n_e][2] */, float *inv_a_odd_ri /* [n_o][2] */);

/* Batched mixed precision: the low-precision GCR on a BLOCK of k Fields (csrc/gcr32_multi.hip), 1 <= k <= 16, columns interleaved
 * as in every multi-vector.  `low` is a LowPrecisionGCR of the square form (mgcr_gcr32_create), Dirac or matrix form; its current
 * inner parameters and k32 apply.
 * mgcr_gcr32_apply_multi: column j of Y is y_j ~ A^-1 f_j from the fp32 restarted GCR.  The k inner solves advance in LOCKSTEP and
 * share every launch: the fp32 slab is streamed once per step for all k columns.
 * Rule M1: column j of Y, its step count and its rel_res (mgcr_gcr32_last_multi) are BIT-IDENTICAL to mgcr_op_apply(low, f_j) and
 * mgcr_gcr32_last — for every k, every column position and whatever the other columns do.  Per column the kernels keep the single
 * kernels' row-to-thread maps, grids, reduction trees and element-wise expressions (one copy of each, shared by both files).
 * Freezing: every column has its own state (stop words, step count, <Ap_i, Ap_i>) and its own partial slabs.  A column stops on its
 * tolerance, on an exactly zero <Ap, Ap> or on f_j = 0; a column that has stopped is frozen — every later store to it is masked.
 * `active`: bit j set — column j takes part; bit j clear — column j performs 0 steps and y_j = 0 (the batched form of the gate the
 * single apply gets from its outer solve; its rel_res is that of 0 steps).  Bits at or above k: MGCR_ERR_INVALID.
 * Launch count: fixed, whatever the data — per step an apply, a dots (not in the step that opens a restart cycle), a build and an
 * update launch, plus an entry and an exit launch: 4 max_iter + 2 - ceil(max_iter / restart) per batched apply.  No host round
 * trip, no atomics, no graph capture.
 * Storage: r, Ar, x and 2 * restart slot blocks of nv * k float2 (nv = n rounded up to 4), held planar (column c of a vector at
 * [c nv, c nv + n), the single solve's layout per column), a second copy of r of nv * k float2 with the columns interleaved (what the
 * k-wide matrix apply gathers from), the partial slabs and the states belong to the operator: allocated by the first batched apply
 * of width k, reallocated — behind a stream synchronisation — when k or restart has changed, freed by mgcr_op_destroy.
 * Counters (mgcr_stat): "gcr32_multi_applies" = batched applies enqueued, "gcr32_multi_steps" = the lockstep steps those enqueued
 * (max_iter each); "gcr32_applies" and "gcr32_steps" do not move.
 * MGCR_ERR_UNSUPPORTED: the even-odd form (mgcr_gcr32_create_eo).  MGCR_ERR_INVALID: not a low-precision GCR, a null handle, F and
 * Y of different shape or the same block, rows != n, `active` bits at or above k.  mgcr_op_apply_multi, mgcr_gcr_solve_multi and
 * the queues go on refusing the operator (above) as the operator they apply or solve on; mgcr_gcr_solve_multi takes it in its
 * right_precond slot with flexible = 1, where this batched apply is the inner solve.
 * mgcr_gcr32_last_multi: ONE synchronisation; steps performed and last fp32 |r| / |f| of each column of the last batched apply
 * that was enqueued, by this call or by mgcr_gcr32_solve_multi (a solve in which no column was ever active enqueues none);
 * MGCR_ERR_INVALID before the operator's first batched apply.
 *
 * mgcr_gcr32_solve_multi: the batched mixed solve, fp64 DEFECT CORRECTION around the k-wide inner solve.  Per column, driven by the
 * host between launches: r = b - A x (without use_x0: x = 0, r = b); hist[j][0] = |r_j| / |b_j|; at outer step t = 1, 2, ... the
 * active columns are those with |r_j|^2 > tol^2 |b_j|^2 (a column with b_j = 0 is never active and counts as converged at 0
 * steps); when none is active or t > max_outer the solve ends; else E = mgcr_gcr32_apply_multi(low, R, active), x_j = x_j + e_j on
 * the active columns, r_j = b_j - (A x)_j from the k-wide fp64 apply (mgcr_op_apply_multi), hist[j][t] = |r_j| / |b_j| and
 * n_outer[j] = t for the active columns.  A column that has converged keeps its x, its history and its count.  One
 * synchronisation per outer step (the k norms).  hist: [k][hist_cap] or NULL; converged[j] = 1 when column j's last residual meets
 * the tolerance.
 * Rule M2: x, history, n_outer and converged of column j are BIT-IDENTICAL to the same loop written with the single-Field entry
 * points on column j alone — mgcr_op_apply(A), mgcr_add_scaled(r, b, -1, t), mgcr_norm2, mgcr_op_apply(low), mgcr_axpy(1, e, x) —
 * wherever mgcr_op_apply_multi is bit-identical to the single apply: every storage form.
 * A: whatever mgcr_op_apply_multi takes on one GPU, with dim == n.  MGCR_ERR_UNSUPPORTED: a MultiDiracOp or MultiEvenOddDiracOp (a
 * shift per column against the one k32 would not contract), distributed operators, GCR or MG objects, a low-precision GCR as A, an
 * even-odd `low`.  MGCR_ERR_INVALID: max_outer < 0, tol < 0, null handles, B and X of different shape or the same block, rows != n.
 * The work blocks (R, E, A X) belong to `low` and are kept between calls while k stays. */
int mgcr_gcr32_apply_multi(mgcr_op_t low, mgcr_mvec_t F, mgcr_mvec_t Y, uint32_t active /* bit j: column j takes part */);
int mgcr_gcr32_last_multi(mgcr_op_t low, int32_t *n_iter /* [k] */, double *rel_res /* [k] */);   /* one synchronisation */
int mgcr_gcr32_solve_multi(mgcr_op_t A, mgcr_op_t low, double tol, int32_t max_outer, int32_t use_x0,
                           mgcr_mvec_t B, mgcr_mvec_t X, double *hist /* [k][hist_cap] or NULL */, int32_t hist_cap,
                           int32_t *n_outer /* [k] */, int32_t *converged /* [k] */);

/* ---- MG: src/MG.h, src/Mesh.h, src/SolverParam.h:38-59 ------------------------------------ */
typedef struct mgcr_mg_param {
    /* MG_Param::mesh + spacetime mask (src/SolverParam.h:41,47): row-major mesh of the fine
     * operator; dimensions with blocked[d] != 0 are cut into blocks of edge subblock_dim
     * (Mesh::blocking, src/Mesh.h:236-298), the others (spinor, colour) stay inside an aggregate.
     * The reference hard-wires 4 blocked dimensions; 1..4 are accepted here. */
    int32_t ndim;
    int64_t dims[8];
    int32_t blocked[8];
    int64_t subblock_dim;    /* MG_Param::subblock_dim */
    /* near-null vectors the prolongator is built from, [n_vec][N] interleaved re/im on the host.
     * (The reference computes n_eigen vectors by inverse iteration and doubles them by chirality,
     * src/MG.h:90-122,316-345; the host mirror does that and passes the 2*n_eigen vectors in.) */
    int32_t n_vec;
    const double *vecs_ri;
    int32_t n_level;         /* MG_Param::n_level = number of COARSE grids (1 = the reference's
                                two-level method; the reference stores it and never reads it) */
    mgcr_gcr_param smoother; /* GCR_Param of MG_Param::smoother_solver (max_iter = sweeps) */
    mgcr_gcr_param coarse;   /* GCR_Param of MG_Param::coarse_solver (coarsest level) */
    double damping;          /* x += damping * P x_c; the reference hard-codes 0.1 (src/MG.h:426) */
    /* extension (0 = the reference's behaviour: the coarsest system goes to `coarse`, src/MG.h:424): when the coarsest
     * level has at most this many unknowns (limit 2048) it is solved DIRECTLY — its operator is inverted once at set-up
     * (dense Gauss-Jordan with partial pivoting on the device) and every cycle applies the inverse with one mat-vec */
    int32_t coarse_direct_rows;
} mgcr_mg_param;

/* MG(Operator*, MG_Param*) + initialise (src/MG.h:131-285): aggregates, block-local prolongator
 * with per-aggregate Gram-Schmidt, Galerkin coarse operators for every level.  A must be a
 * Sparse or a DiracOp.  The result is an Operator whose apply is the corrected V-cycle described
 * in DESIGN.md (MG::operator() of the reference returns uninitialised memory, src/MG.h:124-129). */
int mgcr_mg_create(mgcr_op_t A, const mgcr_mg_param *param, mgcr_op_t *out);
/* number of operator levels, and per level: dimension, vectors per aggregate, aggregates */
int mgcr_mg_level_info(mgcr_op_t mg, int32_t level, int64_t *dim, int32_t *ne, int64_t *nagg);
/* MG::restrict / MG::expand between level and level+1 (src/MG.h:347-383) */
int mgcr_mg_restrict(mgcr_op_t mg, int32_t level, mgcr_vec_t fine, mgcr_vec_t coarse);
int mgcr_mg_expand(mgcr_op_t mg, int32_t level, mgcr_vec_t coarse, mgcr_vec_t fine);
/* borrowed handle of the level's operator (level 0 = A, level >= 1 = Galerkin m_coarse, src/MG.h:281) */
int mgcr_mg_level_op(mgcr_op_t mg, int32_t level, mgcr_op_t *out);
/* prolongator of `level` as [n][ne] block-local values plus the aggregate index of every row */
int mgcr_mg_download_prolongator(mgcr_op_t mg, int32_t level, double *pv_ri, int32_t *agg);

/* ---- multi-GPU: one process per GPU, row-block partition (new design — the reference has no
 *      distribution at all) ------------------------------------------ */
typedef struct mgcr_comm_s *mgcr_comm_t;
typedef struct mgcr_plan_s *mgcr_plan_t;
#define MGCR_RCCL_ID_BYTES 128
/* RCCL over xGMI.  Rank 0 obtains an id, the launcher broadcasts the 128 bytes (bench.py does it
 * with torch.distributed), every rank then creates its communicator.  librccl is dlopen()ed on
 * first use, so single-GPU users do not need it. */
int mgcr_rccl_unique_id(void *id128);
int mgcr_comm_create_rccl(int rank, int nranks, const void *id128, mgcr_comm_t *out);
/* Host-staged transport through caller-supplied callbacks (bring-up and tests: lets several ranks
 * share one GPU, or run the partition logic with no GPU at all).  Buffers are host memory, counts
 * are in doubles.  allreduce: in-place sum over all ranks.  exchange: post all sends / receives
 * to the listed peers and complete them. */
typedef int (*mgcr_allreduce_cb)(void *user, double *buf, int64_t count);
typedef int (*mgcr_exchange_cb)(void *user, int32_t npeers, const int32_t *peers, const double *const *send,
                                const int64_t *send_count, double *const *recv, const int64_t *recv_count);
int mgcr_comm_create_host(int rank, int nranks, mgcr_allreduce_cb allreduce, mgcr_exchange_cb exchange, void *user,
                          mgcr_comm_t *out);
int mgcr_comm_destroy(mgcr_comm_t comm);
/* in-place sum over the ranks of `count` host doubles (set-up-time scalars: global dot products of distributed
 * Fields, sizes); collective */
int mgcr_comm_allreduce_sum(mgcr_comm_t comm, double *buf, int32_t count);
/* how the per-iteration scalars are summed over the ranks: 0 host callbacks, 1 RCCL all-reduce, 2 peer-write
 * mailboxes (one kernel folds and exchanges; chosen by a self-test when the first distributed operator is created,
 * MGCR_PEER_ALLREDUCE=0 disables) */
int mgcr_comm_allreduce_kind(mgcr_comm_t comm, int32_t *kind);
/* how a distributed Sparse (mgcr_dcsr_create) exchanges its halo before an apply: 0 host callbacks, 1 RCCL send/recv
 * group, 2 peer-write (one kernel stores the boundary rows into the neighbours' receive slots and waits for theirs;
 * self-tested at creation, MGCR_PEER_HALO=0 disables) */
int mgcr_op_halo_kind(mgcr_op_t op, int32_t *kind);
/* measurement aid (bench.py, N > 1): average microseconds of one in-place device all-reduce of `count` doubles,
 * issued `reps` times back to back on the library stream (collective: every rank must call it) */
int mgcr_comm_bench_allreduce(mgcr_comm_t comm, int32_t count, int32_t reps, double *us_avg);
/* Partition plan of a row block [row0, row0 + nrow_local) of an n_global-row matrix given with
 * GLOBAL column indices: which remote x entries this rank needs (halo), from whom, what it has
 * to send to whom, and where the rows that touch no remote column sit (they can be multiplied
 * while the halo is in flight).  Pure host code: works without a GPU.  Collective over `comm`. */
int mgcr_plan_create(mgcr_comm_t comm, int64_t n_global, int64_t row0, int64_t nrow_local, const int64_t *rowptr,
                     const int64_t *col_global, mgcr_plan_t *out);
int mgcr_plan_info(mgcr_plan_t plan, int64_t *n_halo, int32_t *npeers, int64_t *interior_begin, int64_t *interior_end);
int mgcr_plan_peers(mgcr_plan_t plan, int32_t *peers, int64_t *send_counts, int64_t *recv_counts);
/* column indices in the local numbering: owned -> col - row0, halo -> nrow_local + slot */
int mgcr_plan_local_columns(mgcr_plan_t plan, int64_t *col_local);
int mgcr_plan_send_indices(mgcr_plan_t plan, int32_t peer_slot, int64_t *local_rows);
int mgcr_plan_halo_globals(mgcr_plan_t plan, int64_t *global_cols);
int mgcr_plan_destroy(mgcr_plan_t plan);
/* Row block of a distributed Sparse: Fields it applies to hold this rank's nrow_local entries;
 * apply = halo exchange (overlapped with the interior rows) + local SpMV; GCR on it all-reduces
 * its dot products (2 small all-reduces per iteration).  Collective over `comm`. */
int mgcr_dcsr_create(mgcr_comm_t comm, int64_t n_global, int64_t row0, int64_t nrow_local, const int64_t *rowptr,
                     const int64_t *col_global, const double *val_ri, mgcr_op_t *out);
/* Row block of a distributed HierarchicalSparse (reference apply: src/HierarchicalSparse.h:101-161; the reference has no
 * distribution, SURVEY.md 8(e) "Unstructured (config 5)"): block rows [brow0, brow0 + nbrow_local) of nb_global, block
 * columns GLOBAL, blocks [nblocks][bs][bs] row-major interleaved (re, im), duplicates of a (row, col) pair kept and
 * summed at apply time like the single-GPU operator.  The halo travels at block granularity (bs values per needed block
 * row of x) and the block kernel reads it in place.  Fields hold this rank's nbrow_local * bs entries.  Collective. */
int mgcr_dbcsr_create(mgcr_comm_t comm, int64_t nb_global, int64_t brow0, int32_t nbrow_local, int32_t bs, const int32_t *browptr,
                      const int64_t *bcol_global, const double *blocks_ri, mgcr_op_t *out);

/* ---- measurement helpers (bench.py) ------------------------------------------------------- */
/* runs `reps` applies back to back on the library stream, bracketed by hipEvents there;
 * returns the average milliseconds per apply */
int mgcr_bench_op_apply(mgcr_op_t op, mgcr_vec_t x, mgcr_vec_t y, int32_t reps, double *ms_avg);
/* the same for the k-wide apply (tools/bench_multi_rhs.py) */
int mgcr_bench_op_apply_multi(mgcr_op_t op, mgcr_mvec_t x, mgcr_mvec_t y, int32_t reps, double *ms_avg);
/* In-loop timing of the last solve that ran with profile_spmv = 1: total milliseconds, over its
 * *n_iter iterations, of the three phases of an iteration — [0] alpha / residual update (+ right
 * preconditioner), [1] operator apply (incl. halo exchange) + beta dot products, [2] direction build —
 * from hipEvents recorded on the library stream between the phases.  *fused = 1 when phase 1 ran as
 * the single SpMV+dot kernel. */
int mgcr_gcr_last_profile(double *phase_ms_total, int32_t *n_iter, int32_t *fused);
/* opaque hipEvent-based stopwatch on the library stream */
int mgcr_timer_start(void);
int mgcr_timer_stop(double *ms);

#ifdef __cplusplus
}
#endif
#endif /* MGCR_H */
