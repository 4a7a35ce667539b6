"""Case table, matrix builders and reference model of the direct coarsest solve's tests (a plain module, like tests/multi_rhs_cases.py
— not a test file).

csrc/dense.hip inverts the coarsest operator by Gauss-Jordan elimination with partial pivoting and applies the inverse with one mat-vec
per cycle.  The inverse is reachable through an MG cycle only, so the cases make the coarsest operator a matrix of their choosing: a
one-dimensional blocked mesh (n,), subblock_dim 1, one near-null vector of ones and one coarse level — every aggregate is one row, every
prolongator entry is exactly 1 and the Galerkin operator is the fine matrix bit for bit (checked on the CPU with the oracle in
tests/test_direct_coarse_cases.py, asserted on the device in tests/test_gpu_direct_coarse.py).  One case ("general") does without the
trick: mesh (64, 2), first dimension blocked by 2, two random complex near-null vectors, a DiracOp shift.

The matrices need pivoting: a cyclic shift by s columns with entries 2 e^{i phi}, up to six random entries of size 0.25 per row, a zero
diagonal.  They are well conditioned, yet no diagonal entry is ever the largest of its column, and GCR does not converge on them — the
direct solve is the only coarsest solver for such operators, and `truth` below is its only reference.

The cycle under test: smoother GCR_Param(0, 10, 1, 1e-30) (one step), damping 0.5, with the reference's alpha = <r, Ap> / <Ap, Ap>:

    step(x0): r = b - A x0;  Ap = A r;  alpha = vdot(r, Ap) / vdot(Ap, Ap);  return x0 + alpha r
    x1 = step(0);  r1 = b - A x1;  xc = Ac^-1 (R r1);  x2 = x1 + 0.5 P xc;  y = step(x2)

`model` is these five lines in whatever precision its arguments have; `truth` runs them in np.clongdouble with xc from the float64 inverse
refined against extended-precision residuals; `e_ref` runs them in complex128 with xc = np.linalg.inv(Ac) @ (R r1), the same class of
algorithm as the device's.  The GPU test asserts  e_gpu <= K max(e_ref, u kappa_inf(Ac)),  e = max|y - y*| / max|y*|, u = 2^-52.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as orc

c128, cld = np.complex128, np.clongdouble
U = 2.0 ** -52
DAMPING = 0.5
SMOOTHER = dict(restart=10, max_iter=1, tol=1e-30)        # GCR_Param(0, 10, 1, 1e-30): one step
SLOPPY = dict(restart=10, max_iter=50, tol=1e-2)          # the coarsest GCR of the cycles that keep it
DENSE_MAX_ROWS = 2048                                     # csrc/internal.h
PIVOT_THREADS = 1024                                      # csrc/dense.hip dense_pivot_kernel: the stride of its search
REFINE_ROUNDS = 6
# K of the bound: the smallest power of two that is at least 4 times the largest ratio e_gpu / max(e_ref, u kappa_inf) of the first run
# on an MI355X (tests/golden/observed_direct_coarse.json); the 4 covers LAPACK's blocked LU against an unblocked Gauss-Jordan and the
# smoothers' device summation order.  The largest ratio was 2.118 (pivot-1024).
K = 16.0

# ---- cases ----------------------------------------------------------------------------------------------------------------------
# kind: "pivot" (cyclic shift s, the trick), "tie" (pivot + a column whose two largest entries have equal modulus), "dirac" (the trick
# under a DiracOp, Id - k D), "general" (no trick), "zero_column" / "equal_rows" / "zero_1x1" (singular), "scaled" (a pivot matrix times
# 2^ea, b times 2^eb).  direct: MG_Param(coarse_direct=).  expect: "bound" | "kept" (the GCR stays: bits of the coarse_direct = 0 cycle)
# | "singular".
Case = namedtuple("Case", "id kind n s cplx seed direct expect ea eb k")
DIRAC_K = 0.3 - 0.2j
GENERAL_K = 0.4 + 0.3j


def _case(id, kind, n, s=0, cplx=True, seed=0, direct=DENSE_MAX_ROWS, expect="bound", ea=0, eb=0, k=None):
    return Case(id, kind, n, s, cplx, seed, direct, expect, ea, eb, k)


def shift_of(n):
    """s: the column of row i's large entry is i + s.  Above 1024 rows n - s >= 1024: the pivot of column k < s sits n - s rows below k."""
    return {1: 0, 1025: 1, 1500: 400, 2048: 1000}.get(n, max(1, n // 3))


def _sizes():
    out = []
    for i, n in enumerate((1, 2, 3, 5, 63, 64, 255, 1023, 1024, 1025, 1500, 2048)):
        out.append(_case("pivot-%d" % n, "pivot", n, shift_of(n), cplx=i % 2 == 0 or n > 1024, seed=n))
    for n in (65, 257):
        out.append(_case("pivot-%d-real" % n, "pivot", n, shift_of(n), cplx=False, seed=n))
        out.append(_case("pivot-%d-complex" % n, "pivot", n, shift_of(n), cplx=True, seed=n + 1))
    out.append(_case("dirac-257", "dirac", 257, shift_of(257), seed=259, k=DIRAC_K))
    return out


# column 0 of the tie case: 5 in place of the shift's entry (row n - s = 87) and 3 + 4i 64 rows above it — |.|^2 = 25 both, exactly; at
# step 0 threads 23 and 87 of the search hold them, and meet at stride 64 of the LDS tree
TIE_ROWS = (23, 87)
TIE_VALUES = (3.0 + 4.0j, 5.0)

BOUND_CASES = _sizes() + [_case("tie-130", "tie", 130, shift_of(130), seed=130),
                          _case("general-64x2", "general", 64, 8, seed=7, k=GENERAL_K)]
KEPT_CASES = [_case("limit-2049", "pivot", 2049, 1000, seed=2049, direct=4096, expect="kept"),
              _case("below-direct-257", "pivot", 257, shift_of(257), seed=258, direct=256, expect="kept")]
SINGULAR_CASES = [_case("zero-column-37", "zero_column", 37, shift_of(37), seed=37, expect="singular"),
                  _case("equal-rows-6", "equal_rows", 6, expect="singular"),
                  _case("zero-1x1", "zero_1x1", 1, expect="singular")]
# the issue's scaled cases: A and b times 2^-600 / 2^+600 — and the same matrices with b scaled so that the SMOOTHER stays in range
# (<Ap, Ap> ~ 2^(2 eb + 2 ea)): what these say about dense.hip does not depend on the smoother's dot products
SCALED_AS_STATED = [_case("scaled-down-65", "scaled", 65, shift_of(65), seed=66, ea=-600, eb=-600),
                    _case("scaled-up-65", "scaled", 65, shift_of(65), seed=66, ea=600, eb=600)]
SCALED_IN_RANGE = [_case("scaled-down-65-b-up", "scaled", 65, shift_of(65), seed=66, ea=-600, eb=200),
                   _case("scaled-up-65-b-down", "scaled", 65, shift_of(65), seed=66, ea=600, eb=-200)]
HEALTHY = BOUND_CASES[5]            # pivot-64: the direct case re-run after the singular set-ups


def all_cases():
    return BOUND_CASES + KEPT_CASES + SINGULAR_CASES + SCALED_AS_STATED + SCALED_IN_RANGE


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def pivoting_matrix(n, s, cplx, seed, extras=6, dominant=0.0):
    """dense n x n: A[i, (i + s) % n] = 2 e^{i phi} (real: +-2), min(extras, n - 2) entries of size 0.25 at random columns off the diagonal
    and off the shift, `dominant` on the diagonal (0: the matrix needs pivoting; 16: diagonally dominant, for the model's own check)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), c128)

    def unit(size):
        return np.exp(2j * np.pi * rng.uniform(0, 1, size)) if cplx else rng.choice([-1.0, 1.0], size).astype(c128)

    rows = np.arange(n)
    A[rows, (rows + s) % n] = 2.0 * unit(n)
    m = min(extras, n - 2)
    for i in range(n if m > 0 else 0):
        free = np.setdiff1d(rows, [i, (i + s) % n])
        A[i, rng.choice(free, m, replace=False)] = 0.25 * unit(m)
    if dominant:
        A[rows, rows] = dominant * (0.8 + 0.6j)       # (not a power of two: a 1 x 1 system is then not solved exactly by one step)
    return A


def csr_of(A):
    """(rowptr, col, val) of the stored entries of a dense matrix, columns ascending; an all-zero row keeps one explicit zero"""
    n = A.shape[0]
    mask = A != 0
    mask[~mask.any(axis=1), 0] = True
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=rowptr[1:])
    return rowptr, np.nonzero(mask)[1].astype(np.int64), A[mask]


Problem = namedtuple("Problem", "N dims blocked sub vecs rowptr col val shift A b")


@functools.lru_cache(maxsize=None)
def problem(case, dominant=0.0):
    """The fine system of a case.  A: the fine operator as a dense complex128 matrix (under a shift: Id - k D, rounded once more than the
    device's x - k (D x) — the GPU test takes the coarse operator from the device and the fine one in extended precision, `fine_exact`).
    dominant > 0: the same structure with a dominant diagonal, on which the oracle's coarsest GCR converges."""
    n, rng = case.n, np.random.default_rng(case.seed + 1000)
    dims, blocked, sub, shift = (n,), (1,), 1, None
    if case.kind in ("pivot", "scaled", "tie", "zero_column"):
        S = pivoting_matrix(n, case.s, case.cplx, case.seed, dominant=dominant)
        if case.kind == "tie":
            assert abs(S[TIE_ROWS[1], 0]) == 2.0
            S[TIE_ROWS, 0] = TIE_VALUES
        if case.kind == "zero_column":
            S[:, 11] = 0
        if case.kind == "scaled":
            S = np.ldexp(S.real, case.ea) + 1j * np.ldexp(S.imag, case.ea)
    elif case.kind == "equal_rows":       # rows 0 and 2: step 0 pivots on row 0 (a tie) and leaves row 2 exactly zero
        S = np.array([[3, 6, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0], [3, 6, 0, 0, 0, 0], [0, 0, 0, 0, 4, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 5]], c128)
    elif case.kind == "zero_1x1":
        S = np.zeros((1, 1), c128)
    elif case.kind == "dirac":            # Id - k D is the pivoting matrix up to rounding (its diagonal: 1e-16, not 0)
        T = pivoting_matrix(n, case.s, True, case.seed, dominant=dominant)
        S = (np.eye(n) - T) / case.k
        shift = case.k
    elif case.kind == "general":          # 64 x 2 sites, aggregates of 2 x 2 = 4 consecutive rows: a shift by 8 aggregates
        n = 128
        dims, blocked, sub = (64, 2), (1, 0), 2
        T = pivoting_matrix(n, 4 * case.s, True, case.seed, dominant=dominant)
        S = (np.eye(n) - T) / case.k
        shift = case.k
    else:
        raise ValueError(case.kind)
    rowptr, col, val = csr_of(S)
    A = np.eye(n) - shift * S if shift is not None else S
    b = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    if case.eb:
        b = np.ldexp(b.real, case.eb) + 1j * np.ldexp(b.imag, case.eb)
    ne = 2 if case.kind == "general" else 1
    vecs = rng.uniform(-1, 1, (ne, n)) + 1j * rng.uniform(-1, 1, (ne, n)) if case.kind == "general" else np.ones((1, n), c128)
    return Problem(n, dims, blocked, sub, vecs, rowptr, col, val, shift, A, b)


def fine_exact(p):
    """the fine operator in extended precision: Id - k D with D and k as stored (what the device's x - k (D x) rounds)"""
    if p.shift is None:
        return p.A.astype(cld)
    D = np.zeros((p.N, p.N), cld)
    D[np.repeat(np.arange(p.N), np.diff(p.rowptr)), p.col] = p.val
    return np.eye(p.N, dtype=cld) - cld(p.shift) * D


def prolongator_matrix(pv, agg, dtype=c128):
    """P as a dense n x (nagg ne) matrix: restrict = P^H, expand = P (oracle.mg_restrict / mg_expand, asserted on the CPU)"""
    n, ne = pv.shape
    P = np.zeros((n, (int(agg.max()) + 1) * ne), dtype)
    for k in range(ne):
        P[np.arange(n), agg * ne + k] = pv[:, k]
    return P


def oracle_mg(case, p, coarse):
    """the oracle's cycle of this problem; coarse: oracle.gcr_param of the coarsest GCR"""
    D = orc.csr(p.N, p.N, p.rowptr, p.col, p.val)
    A = orc.dirac(D, p.shift) if p.shift is not None else D
    return orc.MG(A, p.rowptr, p.col, p.val, p.dims, p.blocked, p.sub, p.vecs, 2, orc.gcr_param(**SMOOTHER), coarse, damping=DAMPING,
                  shift=p.shift)


def dense_view(op, n):
    out = np.empty((n, n), c128)
    for j in range(n):
        e = np.zeros(n, c128)
        e[j] = 1.0
        out[:, j] = op(e)
    return out


def unit_columns(n):
    """the unit vectors the level-1 operator is compared with the fine matrix on: all of them up to 257 rows, 16 above"""
    return range(n) if n <= 257 else np.unique(np.linspace(0, n - 1, 16).astype(int))


@functools.lru_cache(maxsize=None)
def host_hierarchy(case, dominant=0.0):
    """(P, Ac) as the CPU sees them: the trick's identity and the fine matrix, or the oracle's prolongator and Galerkin operator"""
    p = problem(case, dominant)
    if case.kind != "general":
        return np.eye(p.N, dtype=c128), p.A
    Mo = oracle_mg(case, p, orc.gcr_param(**SLOPPY))
    pv, agg = Mo.prolongator(0)
    return prolongator_matrix(pv, agg), dense_view(Mo.level_op(1), Mo.level_dim(1))


# ---- the model ------------------------------------------------------------------------------------------------------------------
def model(A, b, P, coarse_solve, damping=DAMPING):
    """the cycle (module docstring) in the precision of A, b and P; coarse_solve(bc) -> xc"""
    def step(x0):
        r = b - A @ x0
        Ap = A @ r
        return x0 + (np.vdot(r, Ap) / np.vdot(Ap, Ap)) * r

    x1 = step(np.zeros_like(b))
    r1 = b - A @ x1
    xc = coarse_solve(P.conj().T @ r1)
    return step(x1 + damping * (P @ xc))


def kappa_inf(Ac, inv):
    return float(np.linalg.norm(Ac, np.inf) * np.linalg.norm(inv, np.inf))


def refined_solve(Ac, inv, rhs, rounds=REFINE_ROUNDS):
    """Ac x = rhs in extended precision: x = inv rhs with the float64 inverse, then `rounds` of x += inv (rhs - Ac x), the residual in
    extended precision.  -> (x, max|rhs - Ac x|)"""
    x = (inv @ rhs.astype(c128)).astype(cld)
    for _ in range(rounds):
        x = x + (inv @ (rhs - Ac @ x).astype(c128)).astype(cld)
    return x, float(np.abs(rhs - Ac @ x).max())


Reference = namedtuple("Reference", "y e_ref kappa floor residual bnorm")


def reference(A_fine, Ac, P, b):
    """y* (np.clongdouble throughout), e_ref of the complex128 model with the LAPACK inverse, kappa_inf(Ac), the refinement's last
    residual and the norm of its right-hand side.  A_fine: extended precision; Ac, P, b: complex128 as the device holds them."""
    inv = np.linalg.inv(Ac)
    seen = {}

    def solve(bc):
        x, res = refined_solve(Ac.astype(cld), inv, bc)
        seen.update(residual=res, bnorm=float(np.abs(bc).max()))
        return x

    y = model(A_fine, b.astype(cld), P.astype(cld), solve)
    y64 = model(A_fine.astype(c128), b, P, lambda bc: inv @ bc)
    scale = float(np.abs(y).max())
    kap = kappa_inf(Ac, inv)
    return Reference(y, float(np.abs(y64 - y).max()) / scale, kap, U * kap, seen["residual"], seen["bnorm"])


def error_of(y, ref):
    return float(np.abs(np.asarray(y).astype(cld) - ref.y).max() / np.abs(ref.y).max())


def bound_of(ref):
    return K * max(ref.e_ref, ref.floor)


@functools.lru_cache(maxsize=None)
def host_reference(case):
    """the reference as the CPU sees the case (the GPU test builds its own from the device's prolongator and coarse operator)"""
    p = problem(case)
    P, Ac = host_hierarchy(case)
    return reference(fine_exact(p), Ac, P, p.b)


# ---- the elimination on the host --------------------------------------------------------------------------------------------------
def rank_squares(v):
    """the modulus dense_pivot_kernel ranked candidates by before scaled matrices were tested: underflows below 2^-537, overflows
    above 2^511"""
    with np.errstate(over="ignore", under="ignore"):
        return v.real * v.real + v.imag * v.imag


def rank_scaled(v):
    """... and the one it ranks by now: the column scaled by the power of two of its largest component first (exact, so the order and
    the ties of a matrix in the normal range are those of rank_squares)"""
    m = max(np.abs(v.real).max(), np.abs(v.imag).max()) if v.size else 0.0
    if not m > 0:
        return np.zeros(v.shape)
    e = -int(np.frexp(m)[1])
    re, im = np.ldexp(v.real, e), np.ldexp(v.imag, e)
    return re * re + im * im


Elimination = namedtuple("Elimination", "inv pivots swaps far")


def gauss_jordan(A, rank=rank_scaled, window=None, swap_identity=True):
    """csrc/dense.hip on the host in float64: [A | I] -> [I | A^-1], step k takes the row p >= k with the largest modulus in column k
    (the smallest p among equals), swaps it into row k, normalises it and eliminates column k from every other row.  None: singular.
    The two mutants of tests/test_direct_coarse_cases.py: window (only the first `window` candidates are searched) and swap_identity
    False (the identity half keeps its rows)."""
    n = A.shape[0]
    M = np.concatenate([A.astype(c128), np.eye(n, dtype=c128)], axis=1)
    pivots = np.empty(n, np.int64)
    for k in range(n):
        cand = M[k:n if window is None else min(n, k + window), k]
        a = rank(cand)
        j = int(np.argmax(a))              # the first of the largest
        if not a[j] > 0:
            return None
        p = pivots[k] = k + j
        piv = M[p, k]
        if p != k:
            cols = slice(None) if swap_identity else slice(0, n)
            M[[k, p], cols] = M[[p, k], cols]
        M[k] = M[k] / piv
        f = M[:, k].copy()
        f[k] = 0
        nz = np.nonzero(f)[0]
        M[nz] -= np.outer(f[nz], M[k])
    d = pivots - np.arange(n)
    return Elimination(M[:, n:].copy(), pivots, int((d != 0).sum()), int((d >= PIVOT_THREADS).sum()))


def blocked_pivots(A, rank=rank_scaled, window=None, nb=64):
    """The pivot sequence of the same elimination for matrices too large for `gauss_jordan` in a test: the rows at or below k see the
    same updates in an LU factorisation, so a right-looking blocked LU with the kernel's pivot rule finds the same pivots (up to
    rounding in near-ties; compared with gauss_jordan on the CPU).  -> Elimination with inv = (U^-1 L^-1)[perm], or None: singular."""
    n = A.shape[0]
    M = A.astype(c128).copy()
    perm = np.arange(n)
    pivots = np.empty(n, np.int64)
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        for k in range(k0, k1):
            a = rank(M[k:n if window is None else min(n, k + window), k])
            j = int(np.argmax(a))
            if not a[j] > 0:
                return None
            p = pivots[k] = k + j
            if p != k:
                M[[k, p]] = M[[p, k]]
                perm[[k, p]] = perm[[p, k]]
            M[k + 1:, k] /= M[k, k]
            M[k + 1:, k + 1:k1] -= np.outer(M[k + 1:, k], M[k, k + 1:k1])
        if k1 < n:
            L11 = np.tril(M[k0:k1, k0:k1], -1) + np.eye(k1 - k0)
            M[k0:k1, k1:] = np.linalg.solve(L11, M[k0:k1, k1:])
            M[k1:, k1:] -= M[k1:, k0:k1] @ M[k0:k1, k1:]
    L = np.tril(M, -1) + np.eye(n)
    inv = np.empty((n, n), c128)
    inv[:, perm] = np.linalg.solve(np.triu(M), np.linalg.inv(L))      # A[perm] = L U
    d = pivots - np.arange(n)
    return Elimination(inv, pivots, int((d != 0).sum()), int((d >= PIVOT_THREADS).sum()))


FAITHFUL_MAX_ROWS = 257     # gauss_jordan up to here (well under a second), blocked_pivots above


@functools.lru_cache(maxsize=None)
def host_elimination(case):
    _, Ac = host_hierarchy(case)
    return gauss_jordan(Ac) if Ac.shape[0] <= FAITHFUL_MAX_ROWS else blocked_pivots(Ac)
