"""Case table of the queued even-odd scan (mgcr_eo_solve_queue) — a plain module like tests/evenodd_multi_cases.py, on whose cases
and numpy models it builds.  tests/test_evenodd_queue_cases.py checks the premises on the model (CPU);
tests/test_gpu_evenodd_queue.py runs the same ladders on the device and asserts the same premises on the device's own single solves.

A LADDER is (case, hopping parameters, restart, tol, max_iter, widths).  The premise of a ladder at a width (1 < width < number of
systems: a queue of one column, or one as wide as the list, never refills a slot beside a running column): in the schedule that
tests/queue_cases.py derives from the systems' iteration counts
  * a system is admitted after step 0 while another column is still running, and
  * a column is retired at a boundary of the restart cycle at which another column goes on.
Without both a test would pass although admission or retirement touched a neighbour's column.  The device's counts differ from
the model's, so the ladders leave room: the model's counts end in at least three different restart cycles."""
import functools
from collections import namedtuple

import numpy as np

from tests import evenodd_cases as ec
from tests import evenodd_multi_cases as emc
from tests import queue_cases as qc

Ladder = namedtuple("Ladder", "case ks restart tol max_iter widths")


def spread(name, count, complex_at=None):
    """`count` hopping parameters k0 * (0.3 .. 1.0), k0 the case's own; entry complex_at gets an imaginary part"""
    k0 = emc.case_k(name)
    ks = [complex(k0 * f) for f in np.linspace(0.3, 1.0, count)]
    if complex_at is not None:
        ks[complex_at] = ks[complex_at] * (1 + 0.3j)
    return ks


SAMPLE_LONGEST_FIRST = [0.20, 0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18]
SAMPLE_SHUFFLED = [0.15, 0.20, 0.05, 0.18, 0.10, 0.15 + 0.05j]
assert sorted(map(complex, SAMPLE_LONGEST_FIRST), key=abs) == sorted(map(complex, emc.LADDER), key=abs)
assert sorted(map(complex, SAMPLE_SHUFFLED), key=abs) == sorted(map(complex, emc.LADDER), key=abs)
SAMPLE_WIDTHS = (1, 2, 3, 6, 16)

LADDERS = {
    # 1: the sample ladder (tests/evenodd_multi_cases.py), in the given order, longest first and shuffled
    "sample": Ladder("sample", list(emc.LADDER), emc.LADDER_RESTART, emc.LADDER_TOL, emc.LADDER_MAX_ITER, SAMPLE_WIDTHS),
    "sample_longest_first": Ladder("sample", SAMPLE_LONGEST_FIRST, emc.LADDER_RESTART, emc.LADDER_TOL, emc.LADDER_MAX_ITER, SAMPLE_WIDTHS),
    "sample_shuffled": Ladder("sample", SAMPLE_SHUFFLED, emc.LADDER_RESTART, emc.LADDER_TOL, emc.LADDER_MAX_ITER, SAMPLE_WIDTHS),
    # 2: more systems than 16
    "scalar20": Ladder("scalar", spread("scalar", 20, 7), 5, 1e-10, 200, (4,)),
    "chain20": Ladder("chain", spread("chain", 20, 7), 5, 1e-10, 200, (3,)),
    # 3: x on entry (n_e != n_o on open4d)
    "sample_x0": Ladder("sample", list(emc.LADDER), 5, 1e-10, 200, (3,)),
    "open4d_x0": Ladder("open4d", spread("open4d", 6, 2), 5, 1e-10, 200, (3,)),
    # 4: the storage forms of the halves
    "long": Ladder("long", spread("long", 6, 2), 5, 1e-10, 200, (2,)),
    "lanes": Ladder("lanes", spread("lanes", 6, 2), 5, 1e-10, 200, (2,)),
    # (these two converge in 6 .. 15 steps of the model, and two_parts has halves of 8 rows: cycles of 2 steps spread them over 5 boundaries)
    "grid2d_const": Ladder("grid2d_const", spread("grid2d_const", 6, 2), 2, 1e-10, 200, (2,)),
    "scalar_ti": Ladder("scalar_ti", spread("scalar_ti", 6, 2), 2, 1e-10, 200, (2,)),
    "two_parts": Ladder("two_parts", spread("two_parts", 6, 2), 2, 1e-10, 200, (2,)),
}
DISTINCT_RHS = ("scalar20", "chain20", "open4d_x0", "long", "lanes", "grid2d_const", "scalar_ti", "two_parts")


def rhs_of(name, s):
    """the full right-hand side of system s of ladder `name`: one for all systems, or one per system"""
    lad = LADDERS[name]
    n = emc.case(lad.case).n
    return ec.rhs(n, 900 + s) if name in DISTINCT_RHS else ec.rhs(n)


def x0_of(name, s):
    lad = LADDERS[name]
    return 0.01 * ec.rhs(emc.case(lad.case).n, 950 + s)


def premise(its, width, restart):
    """(a system is admitted after step 0 beside a running column, a column retires at a boundary at which another goes on) in the
    schedule of tests/queue_cases.py for these iteration counts"""
    sched, _ = qc.schedule(its, width, restart)
    admit = {s: g for s, _, g in sched}
    end = {s: admit[s] + its[s] for s in admit}                         # the step after which system s has stopped
    freed = {s: -(-end[s] // restart) * restart for s in admit}        # the boundary at which its slot is drained
    beside = lambda t, step: admit[t] < step < end[t]                   # noqa: E731  system t is in a slot and still running at `step`
    admitted = any(admit[s] > 0 and any(beside(t, admit[s]) for t in admit if t != s) for s in admit)
    retired = any(any(beside(t, freed[s]) for t in admit if t != s) for s in admit)
    return admitted, retired


def cycles_spread(its, restart):
    return len({-(-it // restart) for it in its})


def interior_widths(lad):
    return [w for w in lad.widths if 1 < w < len(lad.ks)]


@functools.lru_cache(maxsize=None)
def model_stops(name):
    """iteration counts of the numpy model (tests/evenodd_cases.gcr on the Schur system, x0 = 0) for every system of the ladder"""
    lad = LADDERS[name]
    c, m = emc.case(lad.case), emc.case_plan(lad.case)
    out = []
    for s, k in enumerate(lad.ks):
        bhat = ec.prepare(m, k, rhs_of(name, s))
        out.append(ec.gcr(lambda v, k=k: ec.schur_apply(m, k, v), bhat, lad.restart, lad.tol, lad.max_iter)[2])
    return out
