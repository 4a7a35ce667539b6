"""Case table of the low-precision GCR's tests (a plain module, like tests/evenodd_cases.py — not a test file): the operators, a numpy
model of the host plan (csrc/gcr32_plan.h), of the fp32 matrix apply, of the inner GCR and of the fp64 flexible outer GCR.

The model follows the header comment of mgcr_gcr32_create (include/mgcr.h) operation by operation.  Real and imaginary parts are
separate arrays of the working type `dt` (np.float32: the device's arithmetic; np.float64: "the same algorithm in fp64") and every
product, sum and difference is one numpy operation of that type — no complex64 multiply, nothing fused.  Dot products convert to
double first.  Only the ORDER of the fp64 sums differs from the device (numpy's pairwise sum against the workgroup trees).

tests/test_gcr32_cases.py (CPU) checks the premises on the model alone; tests/test_gcr32_plan.py runs the C++ plan against the model;
tests/test_gpu_gcr32.py runs the device against both.
"""
import functools
from collections import namedtuple

import numpy as np

from mgpreconditionedgcr_amd import problems
from tests import evenodd_cases as eoc

c128 = np.complex128
f32, f64 = np.float32, np.float64
TILE = 1024                    # rows per workgroup of the apply kernel (G32_TILE)

Case = namedtuple("Case", "name n rowptr col val k")      # k None: matrix form
Plan = namedtuple("Plan", "n npad W real ell_col ell_val tail_rows tail_ptr tail_col tail_val tile_tail stored_bytes")

# name -> k values (None: matrix form)
CASES = {"a": (0.10, 0.15, 0.18), "b": (None,), "c": (None,), "d": (0.09, 0.11), "e": (0.18,), "f": (0.45,)}
INNER = ((8, 8, 0.1), (16, 16, 0.01))          # (restart, max_iter, tol)
INNER_TWO_RESTARTS = (4, 10, 0.)               # case a only: tol 0, so every apply runs all 10 steps and crosses two restart boundaries
OUTER = dict(restart=5, tol=1e-10, max_iter=400)
LATTICE_D = (4, 4, 4, 6)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(n, rowptr, col, val) of the case's stored matrix"""
    if name == "a":      # the reference's own 3072-row sample
        return eoc.load_sample()
    if name == "b":      # 315 rows: odd n, less than one workgroup, real slab
        n, _, rp, ci, va = problems.poisson3d_box_csr(9, 7, 5)
        return n, rp, ci, va
    if name == "c":      # 31 713 rows: odd n, many workgroups, ragged last one
        n, _, rp, ci, va = problems.poisson3d_box_csr(33, 31, 31)
        return n, rp, ci, va
    if name in ("d", "g"):      # complex slab, 24 entries per row
        n, rp, ci, va = eoc.hopping_lattice(LATTICE_D, 3, True, 31, False)
        if name == "g":  # one value out of float's range: refused, the message names the row
            va = va.copy()
            va[int(rp[G_ROW]) + 2] = 1e300
        return n, rp, ci, va
    if name == "e":      # tail rows, a spread of row lengths
        rp, ci, va = problems.random_csr(3001, 3001, np.random.default_rng(32), min_len=1, max_len=12, long_rows=3, long_len=200)
        return 3001, rp, ci, va
    if name == "f":      # less than one wave
        return eoc.chain_links([(i, i + 1) for i in range(44)], 45, 33)
    raise ValueError(name)


G_ROW = 777


def case(name, k="first"):
    n, rp, ci, va = matrix(name)
    if k == "first":
        k = CASES[name][0]
    return Case(name, n, rp, ci, va, k)


def all_cases():
    return [(name, k) for name in CASES for k in CASES[name]]


def rhs(n, seed=8):
    """values on the 0.001 grid: none of them is a float"""
    return problems.rhs_grid(n, seed)


def rhs_mixed(c):
    """The right-hand side of the case's MIXED solve (Rule C and the step-count premises).  A real operator (cases b, c: the Poisson
    boxes in matrix form) gets the real part of rhs(n): the library's outer GCR keeps the reference's conjugation, alpha =
    <r, Ap> / <Ap, Ap> with the conjugate on r, which is the minimal-residual coefficient only while <r, Ap> is real.  On a real
    symmetric operator that holds exactly for real data, so the outer iteration is a true minimal-residual one and a perturbation of
    the preconditioner's output of relative size e changes the next residual by O(e).  With complex data on the same operator
    every step's alpha is the conjugate of the minimising one, the iteration amplifies perturbations from step to step, and ANY
    1e-7 noise on an fp64 inner solve's output — not only rounding to fp32 — moves the step count (9 x 7 x 5 box, 16 steps at tol
    0.01: 5 outer steps without noise, 6 with; fp32 7): such a count says nothing about fp32.  The complex operators (a, d, e, f)
    keep the complex rhs(n).  Rules A and B use complex inputs on every case, so the real slabs' imaginary lanes stay tested."""
    b = rhs(c.n)
    return b.real + 0j if plan(c).real and c.k is None else b


# ---- the host plan ----------------------------------------------------------------------------------------------------------------
def choose_width(lens, nrow):
    """spmv_layout.h choose_width: the W that minimises 20 W nrow + 40 tail_nnz(W) + 64 tail_rows(W), the first such"""
    maxlen = int(lens.max()) if lens.size else 0
    hist = np.bincount(lens, minlength=maxlen + 1).astype(np.int64)
    rows_ge = np.zeros(maxlen + 2, np.int64)
    for w in range(maxlen, -1, -1):
        rows_ge[w] = rows_ge[w + 1] + hist[w]
    tail = np.zeros(maxlen + 2, np.int64)
    for w in range(maxlen - 1, -1, -1):
        tail[w] = tail[w + 1] + rows_ge[w + 1]
    best, best_cost = maxlen, 1e300
    for W in range(maxlen + 1):
        cost = 20. * float(W) * float(nrow) + 40. * float(tail[W]) + 64. * float(rows_ge[W + 1])
        if cost < best_cost:
            best, best_cost = W, cost
    return best


def bad_row(c):
    """first row with a value that is not finite or overflows float, or -1"""
    with np.errstate(over="ignore"):
        ok = np.isfinite(c.val.real) & np.isfinite(c.val.imag) & np.isfinite(c.val.real.astype(f32)) & np.isfinite(c.val.imag.astype(f32))
    if ok.all():
        return -1
    e = int(np.nonzero(~ok)[0][0])
    return int(np.searchsorted(c.rowptr, e, side="right") - 1)


def plan(c):
    n = c.n
    lens = np.diff(c.rowptr).astype(np.int64)
    W = choose_width(lens, n) if n else 0
    npad = (n + 63) // 64 * 64
    real = bool((c.val.imag == 0).all())
    ell_col = np.full((W, npad), -1, np.int32)
    ell_val = np.zeros((W, npad), np.complex64)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(c.col.size, dtype=np.int64) - c.rowptr[rows]
    with np.errstate(over="ignore"):
        v32 = c.val.real.astype(f32) + 1j * c.val.imag.astype(f32)
    v32 = v32.astype(np.complex64)
    inell = pos < W
    ell_col[pos[inell], rows[inell]] = c.col[inell]
    ell_val[pos[inell], rows[inell]] = v32[inell]
    tail_rows = np.nonzero(lens > W)[0].astype(np.int32)
    tail_ptr = np.zeros(tail_rows.size + 1, np.int32)
    np.cumsum(lens[tail_rows] - W, out=tail_ptr[1:])
    tail_col = c.col[~inell].astype(np.int32)
    tail_val = v32[~inell]
    ntiles = (n + TILE - 1) // TILE
    tile_tail = np.searchsorted(tail_rows, np.arange(ntiles + 1, dtype=np.int64) * TILE).astype(np.int32)
    vb = 4 if real else 8
    stored = W * npad * (4 + vb) + tail_col.size * (4 + vb) + tail_rows.size * 8 + tile_tail.size * 4
    return Plan(n, npad, W, real, ell_col, ell_val, tail_rows, tail_ptr, tail_col, tail_val, tile_tail, int(stored))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
class Model:
    """The case's operator in the working type dt: apply(xr, xi) -> (yr, yi).  fold_tail: the MUTANT that adds a row's tail into the
    first accumulator."""

    def __init__(self, c, dt=f32, fold_tail=False):
        self.c, self.dt, self.fold_tail = c, dt, fold_tail
        self.p = plan(c)
        self.n = c.n
        lens = np.diff(c.rowptr)
        self.lens = lens
        self.vr, self.vi = c.val.real.astype(dt), c.val.imag.astype(dt)
        self.set_k(c.k)

    def set_k(self, k):
        self.k = k
        if k is not None:
            self.kr, self.ki = self.dt(complex(k).real), self.dt(complex(k).imag)

    def _entry(self, e, xr, xi, rows, sr, si):
        """s[rows] += val[e] * x[col[e]], one stored entry e per listed row"""
        ar, ai = self.vr[e], self.vi[e]
        br, bi = xr[self.c.col[e]], xi[self.c.col[e]]
        if self.p.real:
            sr[rows] = sr[rows] + ar * br
            si[rows] = si[rows] + ar * bi
        else:
            sr[rows] = sr[rows] + (ar * br - ai * bi)
            si[rows] = si[rows] + (ar * bi + ai * br)

    def row_sums(self, xr, xi):
        n, W, rp, lens = self.n, self.p.W, self.c.rowptr, self.lens
        sr, si = np.zeros(n, self.dt), np.zeros(n, self.dt)
        for w in range(W):
            rows = np.nonzero(lens > w)[0]
            self._entry(rp[rows] + w, xr, xi, rows, sr, si)
        for t in self.p.tail_rows:
            t = int(t)
            one = np.array([0])
            if self.fold_tail:
                ur, ui = sr[t:t + 1], si[t:t + 1]
            else:
                ur, ui = np.zeros(1, self.dt), np.zeros(1, self.dt)
            for e in range(int(rp[t]) + W, int(rp[t + 1])):
                self._entry(np.array([e]), xr, xi, one, ur, ui)
            if not self.fold_tail:
                sr[t] = sr[t] + ur[0]
                si[t] = si[t] + ui[0]
        return sr, si

    def apply(self, xr, xi):
        sr, si = self.row_sums(xr, xi)
        if self.k is None:
            return sr, si
        return xr - (self.kr * sr - self.ki * si), xi - (self.kr * si + self.ki * sr)

    def apply_c128(self, x):
        """y = fp64(A_dt dt(x)): what mgcr_gcr32_apply_matrix returns"""
        yr, yi = self.apply(x.real.astype(self.dt), x.imag.astype(self.dt))
        return yr.astype(f64) + 1j * yi.astype(f64)


def apply_f64(c, x):
    """the fp64 operator on a complex128 vector (A x or x - k D x), and sum |a_ij| |x_j| per row"""
    rows = np.repeat(np.arange(c.n, dtype=np.int64), np.diff(c.rowptr))
    s = np.zeros(c.n, c128)
    np.add.at(s, rows, c.val * x[c.col])
    mag = np.bincount(rows, np.abs(c.val) * np.abs(x[c.col]), c.n)
    return (s if c.k is None else x - c.k * s), mag


def dotc(ar, ai, br, bi):
    """<a, b> = sum conj(a) b, every operand converted to double first"""
    ar, ai, br, bi = ar.astype(f64), ai.astype(f64), br.astype(f64), bi.astype(f64)
    return float(np.sum(ar * br + ai * bi)), float(np.sum(ar * bi - ai * br))


def norm2(ar, ai):
    ar, ai = ar.astype(f64), ai.astype(f64)
    return float(np.sum(ar * ar + ai * ai))


def sub_scaled(br, bi, vr, vi, o_r, o_i):
    """o -= b v, un-fused, in the arrays' type"""
    return o_r - (br * vr - bi * vi), o_i - (br * vi + bi * vr)


Inner = namedtuple("Inner", "y n_iter rel margins")


def inner_solve(m, f, restart, max_iter, tol, alpha_mutant=False):
    """The inner GCR of mgcr_gcr32_create on the model m (working type m.dt) from x = 0.  margins: (|r| / |f|) / tol at every
    tolerance test.  alpha_mutant: the MUTANT that rounds <Ap, r> and <Ap, Ap> to the working type before the division."""
    dt = m.dt
    rr, ri = f.real.astype(dt), f.imag.astype(dt)
    xr, xi = np.zeros(m.n, dt), np.zeros(m.n, dt)
    f2 = norm2(rr, ri)
    r2 = f2
    ps, aps, den = [None] * restart, [None] * restart, [0.] * restart
    n_iter, margins = 0, []
    for it in range(1, max_iter + 1):
        if f2 > 0 and tol > 0:
            margins.append(np.sqrt(r2 / f2) / tol)
        if not r2 > tol * tol * f2:
            break
        nd = (it - 1) % restart
        ar_, ai_ = m.apply(rr, ri)
        pr, pi, qr, qi = rr, ri, ar_, ai_
        betas = []
        for j in range(nd):
            nx, ny = dotc(aps[j][0], aps[j][1], ar_, ai_)
            betas.append((dt(nx / den[j]), dt(ny / den[j])))
        for j in range(nd):
            br, bi = betas[j]
            pr, pi = sub_scaled(br, bi, ps[j][0], ps[j][1], pr, pi)
            qr, qi = sub_scaled(br, bi, aps[j][0], aps[j][1], qr, qi)
        aa = norm2(qr, qi)
        arx, ary = dotc(qr, qi, rr, ri)
        if not aa > 0.:
            break
        if alpha_mutant:
            alr, ali = dt(arx) / dt(aa), dt(ary) / dt(aa)
        else:
            alr, ali = dt(arx / aa), dt(ary / aa)
        xr, xi = xr + (alr * pr - ali * pi), xi + (alr * pi + ali * pr)
        rr, ri = sub_scaled(alr, ali, qr, qi, rr, ri)
        r2 = norm2(rr, ri)
        ps[nd], aps[nd], den[nd] = (pr, pi), (qr, qi), aa
        n_iter = it
    rel = float(np.sqrt(r2 / f2)) if f2 > 0 else 0.
    return Inner(xr.astype(f64) + 1j * xi.astype(f64), n_iter, rel, margins)


Outer = namedtuple("Outer", "x n_iter converged inner_total margins inner_margins true_res")


def outer_solve(c, b, precond, restart=5, tol=1e-10, max_iter=400):
    """The library's fp64 restarted GCR (csrc/gcr.hip, oracle/mgcr_oracle.c) with flexible right preconditioning, from x = 0, on the
    case's fp64 operator: z = precond(r) (None: z = r, plain GCR), p = z - sum beta_i p_i, Ap = A z - sum beta_i Ap_i.  It keeps the
    reference's conjugation — alpha = <r, Ap> / <Ap, Ap> and beta_i = <A z, Ap_i> / <Ap_i, Ap_i> with <a, b> = sum conj(a) b, the
    conjugates of the minimal-residual coefficients — and its restart: the direction built by the step that closes a cycle is still
    orthogonalised against the whole cycle and becomes slot 0 of the next.  Stops when |r|^2 <= tol^2 |b|^2.  The preconditioner
    is counted for the steps that use its result (the library enqueues one more apply behind the last residual update)."""
    def prec(r):
        if precond is None:
            return r.copy(), 0, []
        res = precond(r)
        return res.y, res.n_iter, res.margins

    x = np.zeros(c.n, c128)
    r = b.copy()
    b2 = float(np.vdot(b, b).real)
    ps, aps, den = [None] * restart, [None] * restart, [0.] * restart
    z, inner_total, inner_margins = prec(r)
    p, q = z, apply_f64(c, z)[0]
    ps[0], aps[0] = p, q
    cur, iter_count, it, margins, conv = 0, 0, 0, [], False
    while it < max_iter:
        it += 1
        iter_count += 1
        aa = float(np.vdot(q, q).real)
        alpha = np.vdot(r, q) / aa
        den[cur] = aa
        x = x + alpha * p
        r = r - alpha * q
        r2 = float(np.vdot(r, r).real)
        margins.append(np.sqrt(r2 / b2) / tol)
        if r2 <= tol * tol * b2:
            conv = True
            break
        z, ni, mg = prec(r)
        inner_total += ni
        inner_margins += mg
        az = apply_f64(c, z)[0]
        lim = min(restart, iter_count)
        betas = [np.vdot(az, aps[i]) / den[i] for i in range(lim)]
        p, q = z, az
        for i in range(lim):
            p = p - betas[i] * ps[i]
            q = q - betas[i] * aps[i]
        if iter_count % restart == 0:
            iter_count = 0
        cur = iter_count % restart
        ps[cur], aps[cur] = p, q
    ax, _ = apply_f64(c, x)
    return Outer(x, it, conv, inner_total, margins, inner_margins, float(np.linalg.norm(b - ax) / np.linalg.norm(b)))


@functools.lru_cache(maxsize=None)
def mixed(name, k, inner, dt_name, complex_rhs=False):
    """The mixed solve of the case with the inner settings, inner arithmetic float32 or float64 (cached: the tests share it).
    complex_rhs: the complex rhs(n) whatever the operator (COMPLEX_ON_REAL)"""
    c = case(name, k)
    m = Model(c, f32 if dt_name == "f32" else f64)
    restart, max_iter, tol = inner
    return outer_solve(c, rhs(c.n) if complex_rhs else rhs_mixed(c), lambda r: inner_solve(m, r, restart, max_iter, tol), **OUTER)


# The real operators with the COMPLEX right-hand side as well: the full mixed solve with complex data on a real slab.  Two of the four
# are the known exceptions to "fp32 takes fp64's step counts" (rhs_mixed has the cause): (outer, inner) steps in fp32 and in fp64.
# Their counts hang on rounding-size perturbations, so the device's outer count is recorded there, not held to the model's.
COMPLEX_ON_REAL = tuple((name, None, inner) for name in ("b", "c") for inner in INNER)
SENSITIVE = {("b", None, (16, 16, 0.01)): ((7, 78), (5, 57)), ("c", None, (8, 8, 0.1)): ((26, 204), (23, 180))}


def inner_settings(name):
    return INNER + ((INNER_TWO_RESTARTS,) if name == "a" else ())
