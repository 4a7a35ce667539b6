"""Blocks and the numpy model of the flexible batched GCR's tests (a plain module, like tests/gcr32_multi_cases.py — not a test file).

The model is ONE column of mgcr_gcr_solve_multi with a flexible right preconditioner (include/mgcr.h, "Flexible batched GCR"): the
fp64 restarted GCR of gcr32_cases.outer_solve, here with a start vector x0 and with every intermediate x kept, around
gcr32_cases.inner_solve (slot kind (a)).  The device is not compared with the
model's numbers — everything tests/test_gpu_gcr_multi_flex.py compares is bits against the single solve — the model only says WHEN
a column stops, so that the blocks below contain what they claim: columns that stop at different outer steps, inside a restart cycle
with x updates pending and on a step that closes one, while other columns run on.  tests/test_gcr_multi_flex_cases.py (CPU) checks
those premises on the model alone.

A block is a tuple of columns (kind, seed):
    "zero"      b = rhs(n, seed), x0 = 0
    ("mid", t)  b = rhs(n, seed), x0 = the model's x after t steps of the PLAIN fp64 GCR(5) from zero (no preconditioner: cheap, and
                any x0 nearer the solution serves): a column that stops earlier
    "null"      b = 0, x0 = 0 (the zero column)
The duplicate column is a repeated (kind, seed).  Blocks with a "mid" column are solved with use_x0; every block is solved without
it as well (x0 is then ignored, as the reference ignores it).
"""
import functools
from collections import namedtuple

import numpy as np

from tests import gcr32_cases as g

c128 = np.complex128
WIDTHS = (1, 3, 5, 16)                     # one, ragged and full mv_group groups (1 | 4 with one empty lane | 4 + 1 | 4 x 4)
Flex = namedtuple("Flex", "x n_iter converged xs margins")


def flex_solve(c, b, precond, restart, tol, max_iter, x0=None):
    """One column: the library's fp64 restarted GCR with flexible right preconditioning (gcr32_cases.outer_solve's recurrences) from
    x0.  precond(r) -> z.  xs[t]: x after t steps; margins[t - 1]: (|r| / |b|) / tol after step t.  b = 0: the first step's test
    ends the solve (|r|^2 / |b|^2 is not a number, which does not compare greater), not converged only when max_iter == 1."""
    b2 = float(np.vdot(b, b).real)
    if x0 is None:
        x, r = np.zeros(c.n, c128), b.copy()
    else:
        x = x0.copy()
        r = b - g.apply_f64(c, x)[0]
    ps, aps, den = [None] * restart, [None] * restart, [0.] * restart
    z = precond(r)
    p, q = z, g.apply_f64(c, z)[0]
    ps[0], aps[0] = p, q
    cur, iter_count, it, margins, xs = 0, 0, 0, [], [x.copy()]
    max_iter = max(max_iter, 1)
    while it < max_iter:
        it += 1
        iter_count += 1
        aa = float(np.vdot(q, q).real)
        with np.errstate(invalid="ignore", divide="ignore"):
            alpha = np.vdot(r, q) / aa
            den[cur] = aa
            x = x + alpha * p
            r = r - alpha * q
            r2 = float(np.vdot(r, r).real)
            ratio = np.float64(r2) / np.float64(b2)
        xs.append(x.copy())
        margins.append(float(np.sqrt(ratio)) / tol if tol > 0 and ratio == ratio else 0.)
        if not ratio > tol * tol:
            break
        if it == max_iter:
            break
        z = precond(r)
        az = g.apply_f64(c, z)[0]
        lim = min(restart, iter_count)
        betas = [np.vdot(az, aps[i]) / den[i] for i in range(lim)]
        p, q = z, az
        for i in range(lim):
            p = p - betas[i] * ps[i]
            q = q - betas[i] * aps[i]
        if iter_count % restart == 0:
            iter_count = 0
        cur = iter_count % min(restart, max_iter + 1)
        ps[cur], aps[cur] = p, q
    return Flex(x, it, it < max_iter, xs, margins)


# ---- the preconditioners -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name, k):
    return g.Model(g.case(name, k), g.f32)


def low_precond(name, k, inner):
    """slot kind (a): the fp32 inner GCR of the case's operator"""
    m = _model(name, k)
    return lambda r: g.inner_solve(m, r, *inner).y


# ---- the blocks ------------------------------------------------------------------------------------------------------------------------
# outer parameters (restart, max_iter, tol) of the premises
OUTER_5 = (5, 60, 1e-10)            # restart 5
OUTER_3 = (3, 60, 1e-10)            # premise (ii): columns that stop on a closing step
OUTER_1 = (1, 60, 1e-10)            # every step closes a cycle
OUTER_SHORT = (8, 5, 1e-10)         # max_iter < restart: the shortened storage (6 slots); nothing converges in 5 steps
OUTER_LIMIT = (5, 12, 1e-10)        # premise (iv): the solve from zero is still running at step 12

# 16 columns: a zero column at position 2 and a duplicate of column 0 at position 3; "mid" columns stop early
COLUMNS = (("zero", 8), (("mid", 40), 9), ("null", 0), ("zero", 8), (("mid", 24), 9), (("mid", 64), 9), ("zero", 11), (("mid", 96), 10),
           ("zero", 13), (("mid", 16), 10), ("zero", 15), (("mid", 48), 10), ("zero", 17), (("mid", 32), 12), ("zero", 19), (("mid", 80), 12))
PLAIN_STEPS = 96                    # the longest "mid"
PREMISE = ("a", 0.15, g.INNER[0])   # the case, k and inner setting the premises are checked on


@functools.lru_cache(maxsize=None)
def plain_from_zero(name, k, seed):
    """the model's PLAIN GCR(5) on rhs(n, seed) from x = 0, PLAIN_STEPS steps (cached: the blocks share it)"""
    c = g.case(name, k)
    return flex_solve(c, g.rhs(c.n, seed), lambda r: r.copy(), 5, 0., PLAIN_STEPS)


Block = namedtuple("Block", "B X0")


@functools.lru_cache(maxsize=None)
def make_block(name, k, cols):
    """(B, X0) of shape (len(cols), n)"""
    c = g.case(name, k)
    B, X0 = np.zeros((len(cols), c.n), c128), np.zeros((len(cols), c.n), c128)
    for j, (kind, seed) in enumerate(cols):
        if kind == "null":
            continue
        B[j] = g.rhs(c.n, seed)
        if kind != "zero":
            s = plain_from_zero(name, k, seed)
            X0[j] = s.xs[min(kind[1], len(s.xs) - 1)]
    return Block(B, X0)


@functools.lru_cache(maxsize=None)
def model_counts(name, k, inner, outer, cols, use_x0=True):
    """[(n_iter, converged, margins)] of the model per column of the block"""
    c = g.case(name, k)
    blk = make_block(name, k, cols)
    pre = low_precond(name, k, inner)
    out = []
    for j in range(len(cols)):
        s = flex_solve(c, blk.B[j], pre, outer[0], outer[2], outer[1], blk.X0[j] if use_x0 else None)
        out.append((s.n_iter, s.converged, tuple(s.margins)))
    return out


def pending_and_runner(counts, restart, max_iter):
    """premise (i) on a list of stop steps: is there a column that stops inside a cycle (one or more x updates pending) while
    another runs at least `restart` further steps?"""
    inside = [s for s in counts if s % restart != 0 and s < max_iter]
    return any(max(counts) - s >= restart for s in inside)
