"""Case table of the even-odd Schur solve for operators with a site diagonal (a plain module, like tests/evenodd_cases.py — not a
test file): matrices that store a diagonal, built on the hopping cases of tests/evenodd_cases.py, and a numpy model of the plan
(csrc/evenodd_plan.h, evenodd_plan_build_diag), of the coefficients and of the Schur apply, prepare and reconstruct of
csrc/evenodd_diag.hip.

The full operator is A = diag(a) - c H, H the stored off-diagonal part.  Dirac form: A = 1 - k D, a = (1, 0) - k d, c = k; matrix
form: A = M, a = d, c = -1.  d of a row = its stored diagonal entries added in stored order.  Every element-wise product is formed
from real and imaginary parts with separate real operations, (ar br - ai bi, ar bi + ai br), and 1 / a = (ar / den, -ai / den),
den = ar ar + ai ai — the bits the device must show (Rule 1d of include/mgcr.h).

tests/test_evenodd_diag_cases.py (CPU) checks the premises on the model alone; tests/test_evenodd_diag_plan.py runs the C++ plan
against the model; tests/test_gpu_evenodd_diag.py runs the device against both.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import evenodd_cases as ec

c128 = np.complex128

# form: "dirac" (k is the hopping parameter) or "matrix" (k is None); n, rowptr, col, val: the matrix WITH its diagonal entries
DCase = namedtuple("DCase", "name form k n rowptr col val")

DIRAC_ALL = tuple("d_" + name for name in ec.ALL)            # every hopping case with a seeded random complex diagonal
MATRIX = ("poisson_box", "grid2d_const_m", "sample_m")
OTHER = ("sample_twisted", "dup_diag")
APPLY_ONLY = ("chain_zero_even",)
ALL = DIRAC_ALL + MATRIX + OTHER + APPLY_ONLY
PURE = ("open4d", "scalar")                                  # no diagonal at all: Rule 3d
# the cases the solve tests run on: the model alone satisfies the three premises (tests/test_evenodd_diag_cases.py)
SOLVABLE = ("poisson_box", "d_open4d", "d_scalar", "d_sample", "sample_twisted", "d_chain")
POISSON_DIMS = (6, 5, 4)
# H_eo stored one thread per row — the halves are those of the hopping cases —: the fused stage 2 must run on these
FUSED = tuple("d_" + name for name in ("chain", "two_parts", "scalar", "scalar_ti", "grid2d_const", "grid4d_const", "grid2d_varied",
                                       "w7_slab", "w7_ti", "w7_varied")) + ("grid2d_const_m", "dup_diag")
# the (MODE, width / slots) form of diag_stage2_kernel each of them must reach, as FUSED_FORMS of tests/test_gpu_evenodd.py
FUSED_FORMS = {"d_scalar": (0, 8), "d_w7_slab": (0, 7), "d_scalar_ti": (1, 8), "d_w7_ti": (1, 7), "d_grid2d_varied": (2, 4),
               "d_w7_varied": (2, 7), "d_grid2d_const": (3, 5), "d_grid4d_const": (3, 9)}


def with_diagonal(c, rows, vals):
    """The CSR of c plus the diagonal entries (rows[i], rows[i]) = vals[i], every row's entries in ascending column order (a
    repeated row keeps its entries in the order given)"""
    r = np.concatenate([ec.entry_rows(c.n, c.rowptr), np.asarray(rows, np.int64)])
    cc = np.concatenate([c.col, np.asarray(rows, np.int64)])
    v = np.concatenate([c.val, np.asarray(vals, c128)])
    return ec._csr_from_coo(c.n, r, cc, v)


def random_diagonal(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(c128)


def poisson_box():
    n, rowptr, col, val = ec.hopping_lattice(POISSON_DIMS, 1, False, 0, True, axis_real=True)
    hop = ec.Case("box", n, rowptr, col, np.full(col.size, -1.0, c128))
    return with_diagonal(hop, np.arange(n), np.full(n, 6.0, c128))


@functools.lru_cache(maxsize=None)
def case(name):
    if name in DIRAC_ALL:
        base = name[2:]
        c = ec.case(base)
        return DCase(name, "dirac", ec.case_k(base), c.n, *with_diagonal(c, np.arange(c.n), random_diagonal(c.n, 100 + ec.ALL.index(base))))
    if name == "poisson_box":       # 6 x 5 x 4, open: 6 on the diagonal, -1 off it; halves shorter than one wave
        return DCase(name, "matrix", None, int(np.prod(POISSON_DIMS)), *poisson_box())
    if name in ("grid2d_const_m", "sample_m"):    # the matrix itself, made diagonally dominant: d = 1 + sum |row|
        c = ec.case(name[:-2])
        d = 1.0 + np.bincount(ec.entry_rows(c.n, c.rowptr), np.abs(c.val), c.n)
        return DCase(name, "matrix", None, c.n, *with_diagonal(c, np.arange(c.n), d.astype(c128)))
    if name == "sample_twisted":    # twisted mass: a = 1 -+ 0.3 i, alternating from row to row
        c, k = ec.case("sample"), ec.case_k("sample")
        d = np.where(np.arange(c.n) % 2 == 0, 0.3j, -0.3j) / k
        return DCase(name, "dirac", k, c.n, *with_diagonal(c, np.arange(c.n), d))
    if name == "chain_zero_even":   # k = 0.5 and d = 2 on the even row 4: a_e is exactly 0 there
        c = ec.case("chain")
        return DCase(name, "dirac", 0.5, c.n, *with_diagonal(c, [4], [2.0]))
    if name == "dup_diag":          # row 3 stores two diagonal entries, row 6 an explicit zero, the other rows none
        c = ec.case("chain")
        return DCase(name, "dirac", ec.case_k("chain"), c.n, *with_diagonal(c, [3, 3, 6], [0.25 - 0.5j, 1e-3 + 2.0j, 0.0]))
    raise ValueError(name)


def with_k(dc, k):
    return dc._replace(k=k) if dc.form == "dirac" else dc


@functools.lru_cache(maxsize=None)
def rejected(name):
    """singular_odd: (DCase to refuse at creation, DCase that is accepted, the k its set_k must refuse, the full-system row named);
    triangle: (DCase, (row, column) named); matrix_set_k: the DCase whose set_k must be refused"""
    if name == "singular_odd":      # the odd row 1: d = 2, so 1 - k d = 0 exactly at k = 0.5
        c = ec.case("chain")
        mat = with_diagonal(c, [1, 2], [2.0, 0.5])
        return DCase(name, "dirac", 0.5, c.n, *mat), DCase(name, "dirac", 0.25, c.n, *mat), 0.5, 1
    if name == "triangle":
        c, _, entry = ec.rejected("triangle")
        return DCase(name, "dirac", 0.1, c.n, *with_diagonal(c, [0, 1, 2], [0.5, 0.25j, -1.0])), entry
    if name == "matrix_set_k":
        return case("poisson_box")
    raise ValueError(name)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def cplx(re, im):
    out = np.empty(np.shape(re), c128)
    out.real, out.imag = re, im
    return out


def emul(a, b):
    """a (.) b from separate real operations"""
    a, b = np.asarray(a, c128), np.asarray(b, c128)
    return cplx(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def einv(a):
    den = a.real * a.real + a.imag * a.imag
    with np.errstate(divide="ignore", invalid="ignore"):
        return cplx(a.real / den, -a.imag / den)


def strip_case(dc):
    """(the off-diagonal part as an ec.Case, d[n], the number of stored diagonal entries)"""
    rows = ec.entry_rows(dc.n, dc.rowptr)
    on = rows == dc.col
    d = np.zeros(dc.n, c128)
    np.add.at(d, rows[on], dc.val[on])                      # in stored order
    rowptr = np.zeros(dc.n + 1, np.int64)
    np.cumsum(np.bincount(rows[~on], minlength=dc.n), out=rowptr[1:])
    return ec.Case(dc.name, dc.n, rowptr, dc.col[~on], dc.val[~on]), d, int(on.sum())


@functools.lru_cache(maxsize=None)
def strip(name):
    return strip_case(case(name))


@functools.lru_cache(maxsize=None)
def case_plan(name):
    return ec.plan(strip(name)[0])


Coef = namedtuple("Coef", "a c c2 cn")


def coefficients(dc, d):
    """a[n] and the scalars c, c2 = c c, cn = -c as the host forms them"""
    if dc.form == "matrix":
        c = c128(-1.0)
        return Coef(d.copy(), c, c128(emul(c, c)), c128(cplx(-c.real, -c.imag)))
    k = c128(dc.k)
    kd = emul(np.full(d.size, k), d)
    a = cplx(1.0 - kd.real, 0.0 - kd.imag)
    return Coef(a, k, c128(emul(k, k)), c128(cplx(-k.real, -k.imag)))


def scalar_times(s, v):
    return emul(np.full(v.size, c128(s)), v)


def full_apply(dc, x):
    """A x with the matrix as stored (numpy arithmetic: a reference to rounding, not to the bit)"""
    y = ec.csr_apply(ec.Case(dc.name, dc.n, dc.rowptr, dc.col, dc.val), x)
    return y if dc.form == "matrix" else x - dc.k * y


def schur_apply(p, co, x):
    t = emul(einv(co.a[p.odd]), ec.csr_apply(p.oe, x))
    return emul(co.a[p.even], x) - scalar_times(co.c2, ec.csr_apply(p.eo, t))


def prepare(p, co, b):
    return b[p.even] - scalar_times(co.cn, ec.csr_apply(p.eo, emul(einv(co.a[p.odd]), b[p.odd])))


def reconstruct(p, co, b, xe):
    x = np.empty(p.n, c128)
    x[p.even] = xe
    x[p.odd] = emul(einv(co.a[p.odd]), b[p.odd] - scalar_times(co.cn, ec.csr_apply(p.oe, xe)))
    return x


def model(name, k=None):
    """(DCase at k, plan, coefficients)"""
    dc = case(name) if k is None else with_k(case(name), k)
    return dc, case_plan(name), coefficients(dc, strip(name)[1])
