"""EvenOddBlockDiracOp of the C++ mirror (include/mgcr/mgcr_dropin.hpp) through examples/clover_evenodd.cpp: it compiles with g++,
and on the GPU the lines it prints for the sample with seeded Hermitian 12 x 12 site blocks are, digit for digit, those of the
Python EvenOddBlockDiracOp.solve on the same matrix and right-hand side (x0 = 0, GCR(5), 4000 steps, 1e-8); the example itself
checks the result against the full DiracOp solve."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "build", "clover_evenodd")
BS = 12


def seeded(q):
    q = np.asarray(q, np.int64)
    return (((7919 * q) % 1013) / 1013.0 - 0.5) + 1j * (((104729 * q) % 997) / 997.0 - 0.5)


def clover_matrix(n, rowptr, col, val, scale=1.0):
    """D + C as the example stores it: every row its 12 block entries first, then its hops"""
    ns = n // BS
    s, i, j = np.meshgrid(np.arange(ns), np.arange(BS), np.arange(BS), indexing="ij")
    a, b = seeded((BS * s + i) * BS + j + 1), seeded((BS * s + j) * BS + i + 1)
    blocks = scale * (a + np.conj(b)) / 2.0
    lens = np.diff(rowptr)
    new_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens + BS, out=new_ptr[1:])
    ncol = np.empty(new_ptr[-1], np.int64)
    nval = np.empty(new_ptr[-1], np.complex128)
    head = (new_ptr[:-1, None] + np.arange(BS)[None]).ravel()
    ncol[head] = ((np.arange(n) // BS * BS)[:, None] + np.arange(BS)[None]).ravel()
    nval[head] = blocks.reshape(n, BS).ravel()
    rows = np.repeat(np.arange(n), lens)
    tail = new_ptr[rows] + BS + (np.arange(col.size) - rowptr[rows])
    ncol[tail] = col
    nval[tail] = val
    return new_ptr, ncol, nval


def test_example_compiles_with_gxx():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.path.exists(EXE)


def test_example_refuses_a_bad_scale():
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    p = subprocess.run([EXE, "-1"], capture_output=True, text=True, timeout=60)     # (returns before anything touches the device)
    assert p.returncode == 2 and "usage" in p.stderr


def test_the_example_matrix_has_hermitian_site_blocks():
    from tests import evenodd_cases as ec
    c = ec.case("sample")
    rowptr, col, val = clover_matrix(c.n, c.rowptr, c.col, c.val)
    assert rowptr[-1] == c.col.size + c.n * BS
    blk = val[(rowptr[:-1, None] + np.arange(BS)[None]).ravel()].reshape(c.n // BS, BS, BS)
    assert np.array_equal(blk, np.conj(np.swapaxes(blk, 1, 2))) and np.abs(blk).max() > 0.3


@pytest.mark.gpu
def test_lines_equal_the_python_solve(sample_matrix_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    d = os.path.dirname(sample_matrix_path)
    p = subprocess.run([EXE, os.path.basename(sample_matrix_path)], capture_output=True, text=True,
                       env=dict(os.environ, MGCR_SAMPLE_DIR=d), timeout=300, cwd=d)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    from mgpreconditionedgcr_amd import EvenOddBlockDiracOp, Field, GCR_Param, Sparse
    from tests import evenodd_cases as ec
    c = ec.case("sample")
    assert "even-odd: %d rows, %d even, %d odd, bs = 12" % (c.n, c.n // 2, c.n // 2) in p.stdout
    eo = EvenOddBlockDiracOp(Sparse(c.n, c.n, *clover_matrix(c.n, c.rowptr, c.col, c.val)), 0.15, BS)
    x = Field((c.n,)).set_zero()
    eo.solve(Field((c.n,), seeded(np.arange(c.n))), x, GCR_Param(0, 5, 4000, 1e-8, False))
    assert eo.last_converged
    want = ["Step %d residual norm = %.10e" % (i, h) for i, h in enumerate(eo.last_history)]
    assert re.findall(r"^Step \d+ residual norm = \S+$", p.stdout, re.M) == want
    assert "schur: converged after %d steps, |x|^2 = %.10e" % (eo.last_iterations, x.squarednorm()) in p.stdout
    full = re.search(r"^full: converged after (\d+) steps$", p.stdout, re.M)
    assert full and eo.last_iterations < int(full.group(1))
    assert p.stdout.rstrip().endswith("OK")
