"""Case table of the even-odd hopping-parameter scans (MultiEvenOddDiracOp) — a plain module like tests/evenodd_cases.py, whose
cases, plan model and GCR model it builds on.

shifts(name, k): k distinct, partly complex hopping parameters around the case's own (with equal shifts a wrong column index would
pass).  LADDER: the scan of tests/test_evenodd_multi_cases.py and tests/test_gpu_evenodd_multi.py on the golden 4^4 matrix.
bipartite(A, B): D = [[0, A], [B, 0]] with the parity [0] * rows(A) + [1] * rows(B), so that D_eo is A itself and D_oe is B: the
irregular shapes of tests/test_gpu_kscan.py (rows longer than a tail chunk, tail chunks with column windows, several lanes per row)
carry over to the halves."""
import functools

import numpy as np

from mgpreconditionedgcr_amd import problems
from tests import evenodd_cases as ec

c128 = np.complex128

LADDER = [0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18, 0.20]
LADDER_RESTART, LADDER_TOL, LADDER_MAX_ITER = 5, 1e-10, 200
LADDER_MODEL_STOPS = [8, 15, 34, 42, 80, 200]          # where the numpy model stops each column (k = 0.20 would need 283 steps)

# name: (rows per half, random_csr parameters) — tests/test_gpu_kscan.py::IRREGULAR
BIPARTITE = {
    "long": (6000, dict(min_len=1, max_len=7, long_rows=7, long_len=3000)),     # chunk rows and rows longer than a chunk
    "tail": (40000, dict(min_len=3, max_len=40)),                               # tail chunks with column windows (k = 12: 8 + 4)
    "lanes": (700, dict(min_len=30, max_len=45)),                               # several lanes per row
}


def bipartite(A, B):
    """(Case, parity) of D = [[0, A], [B, 0]]; A, B = (rowptr, col, val), A n_e x n_o and B n_o x n_e"""
    (rpa, ca, va), (rpb, cb, vb) = A, B
    ne, no = rpa.size - 1, rpb.size - 1
    rowptr = np.concatenate([rpa, rpa[-1] + rpb[1:]]).astype(np.int64)
    col = np.concatenate([ca + ne, cb]).astype(np.int64)
    val = np.concatenate([va, vb]).astype(c128)
    parity = np.array([0] * ne + [1] * no, np.int8)
    return ec.Case("bipartite", ne + no, rowptr, col, val), parity


@functools.lru_cache(maxsize=None)
def bipartite_blocks(name):
    n, kw = BIPARTITE[name]
    return (problems.random_csr(n, n, np.random.default_rng(n * 8), **kw), problems.random_csr(n, n, np.random.default_rng(n * 8 + 1), **kw))


@functools.lru_cache(maxsize=None)
def bipartite_case(name):
    return bipartite(*bipartite_blocks(name))


def is_bipartite(name):
    return name in BIPARTITE


def case(name):
    return bipartite_case(name)[0] if is_bipartite(name) else ec.case(name)


def parity(name):
    """the caller's parity (bipartite cases), or None: two-coloured"""
    return bipartite_case(name)[1] if is_bipartite(name) else None


@functools.lru_cache(maxsize=None)
def case_plan(name):
    return ec.plan(case(name), parity(name))


def case_k(name):
    """ec.case_k; for a bipartite case its rule for random values: 0.7 over sqrt(entries per row) x rms value"""
    if not is_bipartite(name):
        return ec.case_k(name)
    c = case(name)
    return float(0.7 / (np.sqrt(c.col.size / c.n) * np.sqrt(np.mean(np.abs(c.val) ** 2))))


def shifts(name, k):
    k0 = case_k(name)
    return [k0 * (0.5 + 0.04 * j) + 0.02j * (j % 3) * k0 for j in range(k)]
