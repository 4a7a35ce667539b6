"""EvenOddSparse of the C++ mirror (include/mgcr/mgcr_dropin.hpp) through examples/poisson_evenodd.cpp: it compiles with g++, and on
the GPU the lines it prints for the 6 x 5 x 4 Poisson box are, digit for digit, those of the Python EvenOddSparse.solve on the
`poisson_box` case of tests/evenodd_diag_cases.py with the same right-hand side (x0 = 0, GCR(5), 4000 steps, 1e-10); the example
itself checks the result against the full solve."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "build", "poisson_evenodd")


def example_rhs(n):
    i = np.arange(n, dtype=np.int64)
    return (((7919 * i) % 1013) / 1013.0 - 0.5) + 1j * (((104729 * i) % 997) / 997.0 - 0.5)


def test_example_compiles_with_gxx():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.path.exists(EXE)


def test_example_refuses_a_bad_box():
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    p = subprocess.run([EXE, "0"], capture_output=True, text=True, timeout=60)     # (returns before anything touches the device)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_lines_equal_the_python_solve():
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    from mgpreconditionedgcr_amd import EvenOddSparse, Field, GCR_Param, Sparse
    from tests import evenodd_diag_cases as dc
    c, m = dc.case("poisson_box"), dc.case_plan("poisson_box")
    assert "even-odd: %d rows, %d even, %d odd" % (c.n, m.even.size, m.odd.size) in p.stdout
    eo = EvenOddSparse(Sparse(c.n, c.n, c.rowptr, c.col, c.val))
    x = Field((c.n,)).set_zero()
    eo.solve(Field((c.n,), example_rhs(c.n)), x, GCR_Param(0, 5, 4000, 1e-10, False))
    assert eo.last_converged
    want = ["Step %d residual norm = %.10e" % (i, h) for i, h in enumerate(eo.last_history)]
    assert re.findall(r"^Step \d+ residual norm = \S+$", p.stdout, re.M) == want
    assert "schur: converged after %d steps, |x|^2 = %.10e" % (eo.last_iterations, x.squarednorm()) in p.stdout
    full = re.search(r"^full: converged after (\d+) steps$", p.stdout, re.M)
    assert full and eo.last_iterations < int(full.group(1))
    assert p.stdout.rstrip().endswith("OK")
