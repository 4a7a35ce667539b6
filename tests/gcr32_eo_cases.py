"""Case table of the low-precision GCR in even-odd form (a plain module, like tests/gcr32_cases.py — not a test file): the matrices,
a numpy model of the host plan (csrc/gcr32_eo_plan.h), of the fp32 Schur apply (csrc/gcr32_eo.hip) and of the mixed solve on the
Schur system.

The model follows the header comment of mgcr_gcr32_create_eo (include/mgcr.h) operation by operation.  Each half is a
gcr32_cases.Model (its row sum is the square form's), the diagonal coefficients are those of tests/evenodd_diag_cases.py rounded to
float, and the inner and outer solves are gcr32_cases.inner_solve / outer_solve, the outer one on the fp64 Schur complement written
out as a CSR matrix.

tests/test_gcr32_eo_cases.py (CPU) checks the premises on the model alone; tests/test_gcr32_eo_plan.py runs the C++ plan against the
model; tests/test_gpu_gcr32_eo.py runs the device against both.
"""
import functools
from collections import namedtuple

import numpy as np

from mgpreconditionedgcr_amd import problems
from tests import evenodd_cases as ec
from tests import evenodd_diag_cases as dc
from tests import evenodd_multi_cases as mc
from tests import gcr32_cases as g

c128 = np.complex128
f32, f64 = np.float32, np.float64

# name -> k values (None: matrix form).  (n_e, n_o) where it matters:
#   chain        45 rows (23, 22): halves below one wave; the odd n_e takes the streaming kernels' odd last element
#   two_parts    14 rows: an empty row, n_e != n_o
#   sample       3072 rows (1536, 1536): complex slab, one full tile and a ragged one, set_k between the three k
#   d_open4d, d_scalar, sample_twisted   Dirac form with a complex diagonal (tests/evenodd_diag_cases.py)
#   box_small    Poisson 9 x 7 x 5 in matrix form (158, 157): real slab, c = -1
#   box_many     Poisson 33 x 31 x 31: many tiles
#   bip_long     evenodd_multi_cases' "long" bipartite builder: rows longer than W in both halves, tail rows behind the first tile
CASES = {"chain": ("own",), "two_parts": ("own",), "sample": (0.15, 0.18, 0.15 + 0.05j), "d_open4d": ("own",), "d_scalar": ("own",),
         "sample_twisted": ("own",), "box_small": (None,), "box_many": (None,), "bip_long": ("own",)}
# Rule A only: n_e = 557 056 is 544 tiles against the 512-workgroup cap, so a workgroup takes a second tile
BIG = "lattice_big"
BIG_DIMS = (32, 32, 32, 34)
BIG_K = 0.1
INNER = g.INNER
INNER_TWO_RESTARTS = g.INNER_TWO_RESTARTS        # on the sample at k = 0.15 only
OUTER = g.OUTER
OVERFLOW_ROW = 777                               # case "overflow_value": one off-diagonal value of the sample out of float's range
ZERO_ODD_ROW = 1                                 # case "zero_odd": the odd row 1 of the chain stores d = 2 and k = 0.5

ECase = namedtuple("ECase", "name form k n rowptr col val parity")     # the matrix WITH its diagonal entries; parity None: two-coloured


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(form, the case's own k or None, n, rowptr, col, val, parity)"""
    if name in ("chain", "two_parts", "sample"):
        c = ec.case(name)
        return "dirac", ec.case_k(name), c.n, c.rowptr, c.col, c.val, None
    if name in ("d_open4d", "d_scalar", "sample_twisted"):
        d = dc.case(name)
        return "dirac", d.k, d.n, d.rowptr, d.col, d.val, None
    if name in ("box_small", "box_many"):
        n, _, rp, ci, va = problems.poisson3d_box_csr(*((9, 7, 5) if name == "box_small" else (33, 31, 31)))
        return "matrix", None, n, rp, ci, va.astype(c128), None
    if name == "bip_long":
        c, par = mc.bipartite_case("long")
        return "dirac", mc.case_k("long"), c.n, c.rowptr, c.col, c.val, par
    if name == BIG:
        n, rp, ci, va = ec.hopping_lattice(BIG_DIMS, 1, True, 41, False)
        return "dirac", BIG_K, n, rp, ci, va, None
    raise ValueError(name)


def case(name, k="own"):
    form, k0, n, rp, ci, va, par = matrix(name)
    if form == "matrix":
        k = None
    elif k == "own":
        k = k0
    return ECase(name, form, k, n, rp, ci, va, par)


def all_cases():
    return [(name, case(name, k).k) for name in CASES for k in CASES[name]]


def inner_settings(name, k):
    return INNER + ((INNER_TWO_RESTARTS,) if (name, k) == ("sample", 0.15) else ())


@functools.lru_cache(maxsize=None)
def rejected(name):
    """(ECase to refuse at creation, the full-system row its message names, a word of the message)"""
    if name == "overflow_value":        # a stored value out of float's range
        c = case("sample", 0.15)
        val = c.val.copy()
        val[int(c.rowptr[OVERFLOW_ROW]) + 2] = 1e300
        return c._replace(val=val), OVERFLOW_ROW, "single precision"
    if name == "overflow_a":            # d = 3e38 is a float, k = 2 too, but a = 1 - k d on the even row 4 is not
        c = ec.case("chain")
        rp, ci, va = dc.with_diagonal(c, [4], [3e38])
        return ECase(name, "dirac", 2.0, c.n, rp, ci, va, None), 4, "single precision"
    if name == "overflow_inv":          # a = 1 - k d = (0, -1e-40) on the odd row 3: 1 / a_o = (0, 1e40) is a double, not a float
        c = ec.case("chain")
        rp, ci, va = dc.with_diagonal(c, [3], [2.0 + 2e-40j])
        return ECase(name, "dirac", 0.5, c.n, rp, ci, va, None), 3, "single precision"
    if name == "zero_odd":              # 1 - k d = 0 exactly on the odd row 1
        d = dc.rejected("singular_odd")[0]
        return ECase(name, "dirac", d.k, d.n, d.rowptr, d.col, d.val, None), ZERO_ODD_ROW, "no inverse"
    raise ValueError(name)


REJECTED = ("overflow_value", "overflow_a", "overflow_inv", "zero_odd")


# ---- the host plan ----------------------------------------------------------------------------------------------------------------
EoPlan = namedtuple("EoPlan", "n ne no parity even odd has_diag real halves hplans d coef_f64 stored_bytes")
Coef32 = namedtuple("Coef32", "a_even inv_a_odd c2")           # complex64 arrays (None without a diagonal), complex64 scalar


def half_bytes(p, real):
    vb = 4 if real else 8
    return int(p.W * p.npad * (4 + vb) + p.tail_col.size * (4 + vb) + p.tail_rows.size * 8 + p.tile_tail.size * 4)


@functools.lru_cache(maxsize=None)
def plan_of(name):
    """The plan without k: colouring, halves (gcr32_cases.Case / Plan each, [0] H_eo, [1] H_oe), the ONE real flag, d"""
    c = case(name)
    hop, d, n_diag = dc.strip_case(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val))
    p = ec.plan(hop, c.parity)
    halves = tuple(g.Case(name + "/" + w, h[0], h[2], h[3], h[4], None) for w, h in (("eo", p.eo), ("oe", p.oe)))
    real = bool(all((h.val.imag == 0).all() for h in halves))
    hplans = tuple(g.plan(h)._replace(real=real) for h in halves)
    has_diag = c.form == "matrix" or n_diag > 0
    stored = sum(half_bytes(hp, real) for hp in hplans) + (8 * c.n if has_diag else 0)
    return EoPlan(c.n, p.even.size, p.odd.size, p.parity, p.even, p.odd, has_diag, real, halves, hplans, d, None, int(stored))


def to_c64(z):
    """(float)re, (float)im"""
    with np.errstate(over="ignore"):
        out = np.empty(np.shape(z), np.complex64)
        out.real, out.imag = np.asarray(z).real.astype(f32), np.asarray(z).imag.astype(f32)
    return out


def coefficients(c, p):
    """(dc.Coef in fp64 — a over the FULL system —, Coef32)"""
    co = dc.coefficients(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val), p.d)
    c2 = to_c64(co.c2)
    if not p.has_diag:
        return co, Coef32(None, None, c2)
    return co, Coef32(to_c64(co.a[p.even]), to_c64(dc.einv(co.a[p.odd])), c2)


def refusal(c):
    """None, or (full-system row, word) of the refusal mgcr_gcr32_create_eo must answer — in its order: stored values, the singular
    odd diagonal, a_e, 1 / a_o"""
    cc = g.Case(c.name, c.n, c.rowptr, c.col, c.val, None)
    if g.bad_row(cc) >= 0:
        return g.bad_row(cc), "single precision"
    hop, d, n_diag = dc.strip_case(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val))
    p = ec.plan(hop, c.parity)
    if not (c.form == "matrix" or n_diag > 0):
        return None
    co = dc.coefficients(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val), d)
    inv = dc.einv(co.a[p.odd])
    bad = ~np.isfinite(inv.real) | ~np.isfinite(inv.imag) | (inv == 0)
    if bad.any():
        return int(p.odd[np.nonzero(bad)[0][0]]), "no inverse"
    for rows, v in ((p.even, co.a[p.even]), (p.odd, inv)):
        v32 = to_c64(v)
        bad = ~np.isfinite(v32.real) | ~np.isfinite(v32.imag)
        if bad.any():
            return int(rows[np.nonzero(bad)[0][0]]), "single precision"
    return None


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
class HalfModel(g.Model):
    """gcr32_cases.Model of one half (a rectangular matrix; its plan carries the operator's real flag).  Same arithmetic; the tail
    rows are walked together, entry by entry, so the long rows of the bipartite case stay affordable."""

    def __init__(self, c, hplan, dt, fold_tail=False):
        super().__init__(c, dt, fold_tail)
        self.p = hplan

    def row_sums(self, xr, xi):
        n, W, rp, lens = self.n, self.p.W, self.c.rowptr, self.lens
        sr, si = np.zeros(n, self.dt), np.zeros(n, self.dt)
        for w in range(W):
            rows = np.nonzero(lens > w)[0]
            self._entry(rp[rows] + w, xr, xi, rows, sr, si)
        tr = self.p.tail_rows.astype(np.int64)
        if tr.size:
            if self.fold_tail:
                ur, ui = sr[tr].copy(), si[tr].copy()
            else:
                ur, ui = np.zeros(tr.size, self.dt), np.zeros(tr.size, self.dt)
            for j in range(int((lens[tr] - W).max())):
                sel = np.nonzero(lens[tr] - W > j)[0]
                self._entry(rp[tr[sel]] + W + j, xr, xi, sel, ur, ui)
            if self.fold_tail:
                sr[tr], si[tr] = ur, ui
            else:
                sr[tr] = sr[tr] + ur
                si[tr] = si[tr] + ui
        return sr, si


class EoModel:
    """The Schur complement of the case in the working type dt: apply(xr, xi) -> (yr, yi) on n_e elements.  dt = float32: the
    device's arithmetic (a, 1 / a_o and c2 rounded from fp64); float64: the same algorithm in fp64.  Mutants: no_inv (1 / a_o left
    out of stage 1), c_for_c2 (c in place of c c), fold_tail (the tail folded into the first accumulator)."""

    def __init__(self, c, dt=f32, no_inv=False, c_for_c2=False, fold_tail=False):
        self.c, self.dt, self.no_inv, self.c_for_c2 = c, dt, no_inv, c_for_c2
        self.p = plan_of(c.name)
        self.n = self.p.ne
        self.h = [HalfModel(self.p.halves[i], self.p.hplans[i], dt, fold_tail) for i in (0, 1)]
        self.set_k(c.k)

    def set_k(self, k):
        self.k = k
        c = self.c._replace(k=k)
        co64, co32 = coefficients(c, self.p)
        dt = self.dt
        if dt == f32:
            c2 = to_c64(co64.c) if self.c_for_c2 else co32.c2
            a, inv = co32.a_even, co32.inv_a_odd
        else:
            c2 = co64.c if self.c_for_c2 else co64.c2
            a, inv = (co64.a[self.p.even], dc.einv(co64.a[self.p.odd])) if self.p.has_diag else (None, None)
        self.c2r, self.c2i = dt(c2.real), dt(c2.imag)
        if self.p.has_diag:
            self.ar, self.ai, self.ir, self.ii = a.real.astype(dt), a.imag.astype(dt), inv.real.astype(dt), inv.imag.astype(dt)

    def apply(self, xr, xi):
        ur, ui = self.h[1].apply(xr, xi)
        if self.p.has_diag and not self.no_inv:
            ur, ui = self.ir * ur - self.ii * ui, self.ir * ui + self.ii * ur
        vr, vi = self.h[0].apply(ur, ui)
        wr, wi = self.c2r * vr - self.c2i * vi, self.c2r * vi + self.c2i * vr
        if self.p.has_diag:
            return (self.ar * xr - self.ai * xi) - wr, (self.ar * xi + self.ai * xr) - wi
        return xr - wr, xi - wi

    def apply_c128(self, x):
        """y = fp64(S_dt dt(x)): what mgcr_gcr32_apply_matrix returns"""
        yr, yi = self.apply(x.real.astype(self.dt), x.imag.astype(self.dt))
        return yr.astype(f64) + 1j * yi.astype(f64)


# ---- the fp64 Schur system ------------------------------------------------------------------------------------------------------
def dplan(c):
    """(ec.Plan, dc.Coef) of the case: what dc.schur_apply / prepare / reconstruct take"""
    hop, d, _ = dc.strip_case(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val))
    return ec.plan(hop, c.parity), dc.coefficients(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val), d)


@functools.lru_cache(maxsize=None)
def schur_csr(name, k):
    """S = diag(a_e) - c2 H_eo diag(1 / a_o) H_oe in fp64 as a gcr32_cases.Case (matrix form, columns ascending): the operator
    gcr32_cases.outer_solve runs on"""
    c = case(name, k)
    p, co = dplan(c)
    ne = p.even.size
    _, _, rp0, c0, v0 = p.eo
    _, _, rp1, c1, v1 = p.oe
    inv = dc.einv(co.a[p.odd])
    len1 = np.diff(rp1)
    rows0 = ec.entry_rows(ne, rp0)
    rep = len1[c0]                                           # every entry (i, o) of H_eo meets row o of H_oe
    src = np.repeat(np.arange(c0.size), rep)
    at = np.repeat(rp1[c0] - np.concatenate([[0], np.cumsum(rep)[:-1]]), rep) + np.arange(int(rep.sum()))
    rows = np.concatenate([rows0[src], np.arange(ne)])
    cols = np.concatenate([c1[at], np.arange(ne)])
    vals = np.concatenate([-co.c2 * v0[src] * inv[c0[src]] * v1[at], co.a[p.even]])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    first = np.concatenate([[True], (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])])
    start = np.nonzero(first)[0]
    vals = np.add.reduceat(vals.real, start) + 1j * np.add.reduceat(vals.imag, start)
    rows, cols = rows[start], cols[start]
    rowptr = np.zeros(ne + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=ne), out=rowptr[1:])
    return g.Case(name + "/S", ne, rowptr, cols.astype(np.int64), vals.astype(c128), None)


def rhs(n, seed=8):
    return g.rhs(n, seed)


def rhs_full(c):
    """The full-system right-hand side of the case's mixed solve: real on the real operators in matrix form, complex elsewhere
    (gcr32_cases.rhs_mixed has the reason)"""
    b = rhs(c.n)
    return b.real + 0j if plan_of(c.name).real and c.form == "matrix" else b


def bhat(c):
    p, co = dplan(c)
    return dc.prepare(p, co, rhs_full(c))


@functools.lru_cache(maxsize=None)
def mixed(name, k, inner, dt_name, noise=0.):
    """The mixed solve of the case's Schur system S x_e = bhat_e with the inner settings, inner arithmetic float32 or float64.
    noise: relative size of a seeded random perturbation of every inner result (the SENSITIVE argument)"""
    c = case(name, k)
    m = EoModel(c, f32 if dt_name == "f32" else f64)
    restart, max_iter, tol = inner
    rng = np.random.default_rng(77)

    def prec(r):
        res = g.inner_solve(m, r, restart, max_iter, tol)
        if noise:
            res = res._replace(y=res.y * (1 + noise * (rng.standard_normal(res.y.size) + 1j * rng.standard_normal(res.y.size))))
        return res

    return g.outer_solve(schur_csr(name, k), bhat(c), prec, **OUTER)


# Cases whose float32 and float64 inner solves give different counts: key -> ((outer, inner) in fp32, in fp64).  Each is shown to move
# under 1e-7 noise on the fp64 inner solve as well (tests/test_gcr32_eo_cases.py), so the count says nothing about fp32; the device's
# outer count is recorded there, not held to the model's.
SENSITIVE = {}
