"""Blocks and the numpy model of the batched mixed solve's tests (a plain module, like tests/gcr32_cases.py — not a test file).

The model is the defect-correction loop of mgcr_gcr32_solve_multi (include/mgcr.h) on ONE column: r = b - A x in fp64, e = the inner
GCR of gcr32_cases.inner_solve on r, x += e, until |r|^2 <= tol^2 |b|^2.  It reuses gcr32_cases.Model, inner_solve and apply_f64, so
the inner arithmetic is the single solve's model, operation by operation.

tests/test_gcr32_multi_cases.py (CPU) checks the premises on the model alone; tests/test_gpu_gcr32_multi.py runs the device against
the single entry points bit for bit (Rules M1 and M2) and against the model's outer counts.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import gcr32_cases as g

c128 = np.complex128
TOL = 1e-10
MAX_OUTER = 40
# (name, k) of the Rule M2 cases and of the premises
M2_CASES = (("a", 0.15), ("a", 0.18), ("b", None), ("d", 0.09), ("e", 0.18))
# Rule M1: name -> k (None: matrix form)
M1_CASES = (("f", 0.45), ("b", None), ("d", 0.09), ("e", 0.18), ("a", 0.18), ("c", None))
WIDTHS = (1, 2, 3, 5, 8, 16)
# the ragged block of Rule M1: (case, k, inner setting) — picked on the CPU so that the premise holds (test_gcr32_multi_cases.py)
RAGGED = ("a", 0.15, (8, 6, 0.1))     # 6 steps at the most: the late residuals, which need 7 or 8, miss the tolerance
RAGGED_SEEDS = (8, 9, 10)
RAGGED_RESIDUALS = (1, 2, 6)          # the model solve's residual after that many outer steps

Defect = namedtuple("Defect", "x n_outer converged inner_total hist xs rs inner_iters inner_margins")


def defect_solve(c, m, b, inner, tol=TOL, max_outer=MAX_OUTER, x0=None):
    """One column of mgcr_gcr32_solve_multi on the model m (inner arithmetic m.dt).  xs[t], rs[t]: x and r after t outer steps;
    hist[t] = |r| / |b|; inner_iters[t - 1]: steps of outer step t's inner solve."""
    restart, max_iter, itol = inner
    b2 = float(np.vdot(b, b).real)
    if x0 is None:
        x, r = np.zeros(c.n, c128), b.copy()
    else:
        x = x0.copy()
        r = b - g.apply_f64(c, x)[0]
    r2 = float(np.vdot(r, r).real)
    rel = lambda: float(np.sqrt(r2 / b2)) if b2 > 0 else 0.
    hist, xs, rs, iters, margins = [rel()], [x.copy()], [r.copy()], [], []
    t = 0
    while r2 > tol * tol * b2 and t < max_outer:
        t += 1
        res = g.inner_solve(m, r, restart, max_iter, itol)
        x = x + res.y
        r = b - g.apply_f64(c, x)[0]
        r2 = float(np.vdot(r, r).real)
        hist.append(rel())
        xs.append(x.copy())
        rs.append(r.copy())
        iters.append(res.n_iter)
        margins += res.margins
    return Defect(x, t, not r2 > tol * tol * b2, int(sum(iters)), np.array(hist), xs, rs, iters, margins)


@functools.lru_cache(maxsize=None)
def model(name, k, dt_name):
    return g.Model(g.case(name, k), g.f32 if dt_name == "f32" else g.f64)


@functools.lru_cache(maxsize=None)
def solved(name, k, inner, dt_name="f32", seed=8):
    """The model's solve of rhs(n, seed) from x = 0 (cached: the tests share it)"""
    c = g.case(name, k)
    return defect_solve(c, model(name, k, dt_name), g.rhs(c.n, seed), inner)


# ---- the Rule M2 block: columns that take different outer counts through x0 ------------------------------------------------------------
# kinds: "zero"  x0 = 0;  "three"  the model's x after 3 outer steps;  "done"  the model's converged x (0 outer steps);
#        "null"  b = 0, x0 = 0 (never active, converged at 0 steps)
M2_KINDS = {3: (("three", 8), ("done", 9), ("zero", 10)),
            8: (("zero", 8), ("three", 8), ("done", 8), ("null", 0), ("zero", 9), ("three", 9), ("zero", 8), ("done", 10))}

Block = namedtuple("Block", "B X0 n_outer")


@functools.lru_cache(maxsize=None)
def m2_block(name, k, inner, width):
    """(B, X0, the model's outer count per column), B and X0 of shape (width, n)"""
    c = g.case(name, k)
    B, X0, counts = np.zeros((width, c.n), c128), np.zeros((width, c.n), c128), []
    for j, (kind, seed) in enumerate(M2_KINDS[width]):
        if kind == "null":
            counts.append(0)
            continue
        s = solved(name, k, inner, "f32", seed)
        B[j] = g.rhs(c.n, seed)
        if kind == "zero":
            counts.append(s.n_outer)
        elif kind == "three":
            X0[j] = s.xs[3]
            counts.append(s.n_outer - 3)
        else:
            X0[j] = s.x
            counts.append(0)
    return Block(B, X0, counts)


# ---- the ragged block of Rule M1 ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_block():
    """(F of shape (columns, n), the model's inner step count and last |r| / |f| per column): right-hand sides at several seeds, a zero column, a
    duplicate of column 0 and residuals of successive outer steps of a model solve, whose inner solves differ in length"""
    name, k, inner = RAGGED
    c = g.case(name, k)
    s = solved(name, k, g.INNER[0])
    cols = [g.rhs(c.n, seed) for seed in RAGGED_SEEDS] + [np.zeros(c.n, c128), g.rhs(c.n, RAGGED_SEEDS[0])] + [s.rs[t] for t in RAGGED_RESIDUALS]
    F = np.array(cols, c128)
    m = model(name, k, "f32")
    res = [g.inner_solve(m, f, *inner) for f in F]
    return F, [r.n_iter for r in res], [r.rel for r in res]
