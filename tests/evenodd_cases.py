"""Case table of the even-odd preconditioned DiracOp's tests (a plain module, like tests/multi_rhs_cases.py — not a test file):
the builders of the hopping matrices, and a numpy model of the host plan (csrc/evenodd_plan.h), of the Schur apply and of
restarted GCR.

tests/test_evenodd_cases.py (CPU) checks the premises on the model alone; tests/test_evenodd_plan.py runs the C++ plan against the
model; tests/test_gpu_evenodd.py runs the device against both.

The model of the plan: colour = parity of the breadth-first distance from the component's root in the graph of D + D^T, components
in order of their smallest row, the root even; first offending entry = first in stored order with equal colours at both ends;
even / odd = ascending rows of each colour; half matrices with rows in list order, columns renumbered into the other list and a
row's entries in stored order.
"""
import functools
import gzip
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
c128 = np.complex128

Case = namedtuple("Case", "name n rowptr col val")
Plan = namedtuple("Plan", "n parity even odd index eo oe")     # eo / oe: (nrow, ncol, rowptr, col, val)

ALL = ("sample", "open4d", "chain", "two_parts", "periodic_ti", "scalar", "scalar_ti", "grid2d_const", "grid4d_const", "grid2d_varied",
       "w7_slab", "w7_ti", "w7_varied")
SAMPLE_DIMS = (4, 4, 4, 4, 4, 3)       # (t, z, y, x, spinor, colour)
OPEN4D_DIMS = (3, 3, 5, 7)
PERIODIC_DIMS = (8, 8, 8, 12)
SCALAR_DIMS = (4, 4, 6, 6)             # one unknown per site: rows of 8 entries, stored one thread per row
SCALAR_TI_DIMS = (16, 16, 16, 16)      # ... and halves of 2^15 rows with translation-invariant hops: a dictionary form
NCOMP = 12
# one unknown per site, open boundaries, halves of 2^15 rows (what the dictionary forms need) — built so that every storage form the
# fused stage of a GCR step exists for is reached: constant real hops (one value per axis) make a stencil view — in half-row
# numbering a 2-D grid has the 5 column offsets -Lx/2, -1, 0, 1, Lx/2 (7 slots), a 4-D grid 9 —; values that differ from row to
# row leave a dictionary of the columns only; a first dimension of length 2 makes rows of exactly 7 entries (the width compiled in)
GRID2D_DIMS = (256, 256)
GRID4D_DIMS = (16, 16, 16, 16)
W7_SLAB_DIMS = (2, 8, 8, 8)
W7_DIMS = (2, 32, 32, 32)


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _csr_from_coo(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, np.ascontiguousarray(cols, np.int64), np.ascontiguousarray(vals, c128)


def hopping_lattice(dims, ncomp, periodic, seed, translation_invariant, axis_real=False):
    """Nearest-neighbour hopping matrix on a lattice (sites row-major, ncomp unknowns per site): one random complex
    ncomp x ncomp block per (site, direction, sign) — or per (direction, sign) only; axis_real: one random REAL block per direction,
    the same for both signs —, no diagonal.  Entries of a row in ascending column order."""
    rng = np.random.default_rng(seed)
    dims = tuple(int(d) for d in dims)
    nsite = int(np.prod(dims))
    coords = np.stack(np.unravel_index(np.arange(nsite, dtype=np.int64), dims), axis=1)
    a, b = np.meshgrid(np.arange(ncomp, dtype=np.int64), np.arange(ncomp, dtype=np.int64), indexing="ij")
    rows, cols, vals = [], [], []
    for mu in range(len(dims)):
        axis_blk = rng.uniform(0.5, 1.5, (ncomp, ncomp)) + 0j if axis_real else None
        for sign in (-1, 1):
            c = coords.copy()
            c[:, mu] += sign
            if periodic:
                assert dims[mu] % 2 == 0 and dims[mu] > 2, "a periodic direction must be even (bipartite) and longer than 2"
                c[:, mu] %= dims[mu]
                ok = np.ones(nsite, bool)
            else:
                ok = (c[:, mu] >= 0) & (c[:, mu] < dims[mu])
            src = np.nonzero(ok)[0]
            dst = np.ravel_multi_index(tuple(c[ok].T), dims)
            if axis_real:
                v = np.broadcast_to(axis_blk, (src.size, ncomp, ncomp))
            elif translation_invariant:
                blk = rng.uniform(-1, 1, (ncomp, ncomp)) + 1j * rng.uniform(-1, 1, (ncomp, ncomp))
                v = np.broadcast_to(blk, (src.size, ncomp, ncomp))
            else:
                v = rng.uniform(-1, 1, (src.size, ncomp, ncomp)) + 1j * rng.uniform(-1, 1, (src.size, ncomp, ncomp))
            rows.append((src[:, None, None] * ncomp + a[None]).ravel())
            cols.append((dst[:, None, None] * ncomp + b[None]).ravel())
            vals.append(np.ascontiguousarray(v).ravel())
    return (nsite * ncomp,) + _csr_from_coo(nsite * ncomp, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def chain_links(links, n, seed):
    """Rows joined pairwise by `links` (both directions stored), random complex values"""
    rng = np.random.default_rng(seed)
    links = np.asarray(links, np.int64).reshape(-1, 2)
    rows = np.concatenate([links[:, 0], links[:, 1]])
    cols = np.concatenate([links[:, 1], links[:, 0]])
    vals = rng.uniform(-1, 1, rows.size) + 1j * rng.uniform(-1, 1, rows.size)
    return (n,) + _csr_from_coo(n, rows, cols, vals)


@functools.lru_cache(maxsize=None)
def load_sample():
    """The golden 4^4 matrix (text CSR: `nrow ncol nnz`, the row offsets, then `col (re,im)` per entry)"""
    with gzip.open(os.path.join(GOLDEN, "4x4parsed.txt.gz"), "rt") as f:
        nrow, ncol, nnz = (int(t) for t in f.readline().split())
        assert nrow == ncol
        rowptr = np.empty(nrow + 1, np.int64)
        rowptr[:nrow] = np.array(f.readline().split(), dtype=np.int64)
        rowptr[nrow] = nnz
        body = f.read().replace("(", " ").replace(")", " ").replace(",", " ").split()
    tab = np.array(body[: 3 * nnz], dtype=np.float64).reshape(nnz, 3)
    return nrow, rowptr, tab[:, 0].astype(np.int64), (tab[:, 1] + 1j * tab[:, 2]).astype(c128)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "sample":
        return Case(name, *load_sample())
    if name == "open4d":        # rectangular halves, no multiple of 64, row lengths vary with the boundary
        return Case(name, *hopping_lattice(OPEN4D_DIMS, NCOMP, False, 11, False))
    if name == "chain":         # halves of less than one wave
        return Case(name, *chain_links([(i, i + 1) for i in range(44)], 45, 12))
    if name == "two_parts":     # rows 0..5 a chain, row 6 empty, rows 7..13 a chain whose root (row 7) is even
        return Case(name, *chain_links([(i, i + 1) for i in range(5)] + [(i, i + 1) for i in range(7, 13)], 14, 13))
    if name == "periodic_ti":   # halves of 2^15 rows and more; translation-invariant blocks
        return Case(name, *hopping_lattice(PERIODIC_DIMS, NCOMP, True, 14, True))
    if name == "scalar":        # rows short enough for one thread each: the form whose GCR steps fuse stage 2 with the dot products
        return Case(name, *hopping_lattice(SCALAR_DIMS, 1, True, 16, False))
    if name == "scalar_ti":
        return Case(name, *hopping_lattice(SCALAR_TI_DIMS, 1, True, 17, True))
    if name == "grid2d_const":
        return Case(name, *hopping_lattice(GRID2D_DIMS, 1, False, 18, True, axis_real=True))
    if name == "grid4d_const":
        return Case(name, *hopping_lattice(GRID4D_DIMS, 1, False, 19, True, axis_real=True))
    if name == "grid2d_varied":
        return Case(name, *hopping_lattice(GRID2D_DIMS, 1, False, 20, False))
    if name == "w7_slab":
        return Case(name, *hopping_lattice(W7_SLAB_DIMS, 1, False, 21, False))
    if name == "w7_ti":
        return Case(name, *hopping_lattice(W7_DIMS, 1, False, 22, True))
    if name == "w7_varied":
        return Case(name, *hopping_lattice(W7_DIMS, 1, False, 23, False))
    raise ValueError(name)


def case_k(name):
    """A hopping parameter at which GCR on the case is neither trivial nor hopeless: 0.15 on the sample, else 0.7 over a rough
    estimate of D's spectral radius (sqrt(entries per row) x rms value).  Translation-invariant hops (`scalar_ti`, the constant grids, `w7_ti`) can
    add up in phase, far beyond that estimate: 0.7 over the largest absolute row sum there."""
    if name == "sample":
        return 0.15
    c = case(name)
    if name in ("scalar_ti", "grid2d_const", "grid4d_const", "w7_ti"):
        return float(0.7 / np.bincount(entry_rows(c.n, c.rowptr), np.abs(c.val), c.n).max())
    return float(0.7 / (np.sqrt(c.col.size / c.n) * np.sqrt(np.mean(np.abs(c.val) ** 2))))


def sample_site_parity():
    n = int(np.prod(SAMPLE_DIMS))
    site = np.arange(n, dtype=np.int64) // (SAMPLE_DIMS[4] * SAMPLE_DIMS[5])
    t, z, y, x = np.unravel_index(site, SAMPLE_DIMS[:4])
    return ((t + z + y + x) % 2).astype(np.int8)


@functools.lru_cache(maxsize=None)
def rejected(name):
    """(Case, caller parity or None, the (row, column) the plan must name)"""
    if name == "diagonal":
        c = case("open4d")
        r = 1234
        rows = np.repeat(np.arange(c.n, dtype=np.int64), np.diff(c.rowptr))
        rowptr, col, val = _csr_from_coo(c.n, np.append(rows, r), np.append(c.col, r), np.append(c.val, 0.5 + 0.25j))
        return Case("open4d+diagonal", c.n, rowptr, col, val), None, (r, r)
    if name == "triangle":      # 0 even, 1 and 2 odd: the first stored entry with equal colours is (1, 2)
        return Case(name, *chain_links([(0, 1), (1, 2), (2, 0)], 3, 15)), None, (1, 2)
    if name == "flipped":
        c = case("sample")
        par = sample_site_parity()
        r = 777
        par[r] ^= 1
        # the first entry in stored order that touches row r: in the first row that has r as a column, or r's own first entry
        rows = np.repeat(np.arange(c.n, dtype=np.int64), np.diff(c.rowptr))
        first = np.nonzero((rows == r) | (c.col == r))[0][0]
        return c, par, (int(rows[first]), int(c.col[first]))
    raise ValueError(name)


REJECTED = ("diagonal", "triangle", "flipped")


def rhs(n, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(c128)


# ---- the model of the plan ------------------------------------------------------------------------------------------------------
def entry_rows(n, rowptr):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))


def colour(n, rowptr, col):
    """Breadth-first two-colouring of D + D^T: parity of the distance from the component's root (its smallest row, even)"""
    rows = entry_rows(n, rowptr)
    src = np.concatenate([rows, col])
    dst = np.concatenate([col, rows])
    order = np.argsort(src, kind="stable")
    dst = dst[order]
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ptr[1:])
    parity = np.full(n, -1, np.int8)
    root = 0
    while root < n:
        if parity[root] >= 0:
            root += 1
            continue
        parity[root] = 0
        frontier = np.array([root], np.int64)
        level = 0
        while frontier.size:
            level ^= 1
            lens = ptr[frontier + 1] - ptr[frontier]
            if lens.sum() == 0:
                break
            starts = np.repeat(ptr[frontier] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
            nb = np.unique(dst[starts + np.arange(lens.sum())])
            nb = nb[parity[nb] < 0]
            parity[nb] = level
            frontier = nb
    return parity


def first_conflict(n, rowptr, col, parity):
    rows = entry_rows(n, rowptr)
    bad = np.nonzero(parity[rows] == parity[col])[0]
    return None if bad.size == 0 else (int(rows[bad[0]]), int(col[bad[0]]))


def plan(c, parity=None):
    par = colour(c.n, c.rowptr, c.col) if parity is None else np.asarray(parity, np.int8)
    assert first_conflict(c.n, c.rowptr, c.col, par) is None
    even, odd = np.nonzero(par == 0)[0].astype(np.int64), np.nonzero(par == 1)[0].astype(np.int64)
    index = np.empty(c.n, np.int64)
    index[even] = np.arange(even.size)
    index[odd] = np.arange(odd.size)
    rows = entry_rows(c.n, c.rowptr)
    lens = np.diff(c.rowptr)

    def half(which, lst, ncol):
        m = par[rows] == which
        rp = np.zeros(lst.size + 1, np.int64)
        np.cumsum(lens[lst], out=rp[1:])
        return lst.size, ncol, rp, index[c.col[m]], c.val[m]

    return Plan(c.n, par, even, odd, index, half(0, even, odd.size), half(1, odd, even.size))


@functools.lru_cache(maxsize=None)
def case_plan(name):
    return plan(case(name))


# ---- the model of the operators and of GCR ------------------------------------------------------------------------------------
def csr_apply(h, x):
    """y = A x for A = (nrow, ncol, rowptr, col, val) — or a Case (square)"""
    if isinstance(h, Case):
        h = (h.n, h.n, h.rowptr, h.col, h.val)
    nrow, _, rowptr, col, val = h
    rows = entry_rows(nrow, rowptr)
    prod = val * x[col]
    return np.bincount(rows, prod.real, nrow) + 1j * np.bincount(rows, prod.imag, nrow)


def dirac_apply(c, k, x):
    return x - k * csr_apply(c, x)


def schur_apply(p, k, x):
    return x - (k * k) * csr_apply(p.eo, csr_apply(p.oe, x))


def prepare(p, k, b):
    return b[p.even] + k * csr_apply(p.eo, b[p.odd])


def reconstruct(p, k, b, xe):
    x = np.empty(p.n, c128)
    x[p.even] = xe
    x[p.odd] = b[p.odd] + k * csr_apply(p.oe, xe)
    return x


def gcr(apply, b, restart, tol, max_iter):
    """Restarted GCR from x0 = 0: (x, history relative to |b|, iterations, converged)"""
    x = np.zeros_like(b)
    r = b.copy()
    bn = np.linalg.norm(b)
    hist = [np.linalg.norm(r) / bn]
    it = 0
    while it < max_iter and hist[-1] > tol:
        ps, aps = [], []
        for _ in range(restart):
            p = r.copy()
            ap = apply(p)
            for pj, apj in zip(ps, aps):
                beta = np.vdot(apj, ap) / np.vdot(apj, apj)
                p -= beta * pj
                ap -= beta * apj
            alpha = np.vdot(ap, r) / np.vdot(ap, ap)
            x += alpha * p
            r -= alpha * ap
            ps.append(p)
            aps.append(ap)
            it += 1
            hist.append(np.linalg.norm(r) / bn)
            if it >= max_iter or not hist[-1] > tol:
                break
    return x, np.array(hist), it, bool(hist[-1] <= tol)
