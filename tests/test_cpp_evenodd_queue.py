"""EvenOddDiracOp::solve_queue of the C++ mirror (include/mgcr/mgcr_dropin.hpp) through examples/k_critical_evenodd_queue.cpp: it
compiles with g++, and on the GPU the lines it prints for a four-value hopping-parameter scan of the sample through two columns are,
digit for digit, those of the Python EvenOddDiracOp.solve_queue with the same parameters (rhs = the golden `gcr_rhs` for every
system, x0 = 0, GCR(5), 4000 steps, 1e-10)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "build", "k_critical_evenodd_queue")
KS = [0.18, 0.05, 0.15, 0.10]


def test_example_compiles_with_gxx():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.path.exists(EXE)


def test_example_wants_a_width_and_a_k():
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    p = subprocess.run([EXE, "2"], capture_output=True, text=True, timeout=60)     # (returns before anything touches the device)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_scan_lines_equal_the_python_queued_evenodd_solve(sample_matrix_path, sample_gold):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    d = os.path.dirname(sample_matrix_path)
    p = subprocess.run([EXE, os.path.basename(sample_matrix_path), "2"] + ["%r" % k for k in KS], capture_output=True, text=True,
                       env=dict(os.environ, MGCR_SAMPLE_DIR=d), timeout=300, cwd=d)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    from mgpreconditionedgcr_amd import EvenOddDiracOp, Field, GCR_Param, read_data
    D = read_data(os.path.basename(sample_matrix_path), directory=d)
    n = D.get_dim()
    assert "even-odd: %d rows, %d even, %d odd" % (n, n // 2, n // 2) in p.stdout
    eo = EvenOddDiracOp(D, KS[0])
    b = Field((n,), sample_gold["gcr_rhs"])
    xs = [Field((n,)).set_zero() for _ in KS]
    eo.solve_queue([b] * len(KS), xs, KS, GCR_Param(0, 5, 4000, 1e-10, False), width=2)
    want = ["[%d] Step %d residual norm = %.10e" % (j, i, h) for j in range(len(KS)) for i, h in enumerate(eo.last_history[j])]
    printed = re.findall(r"^\[\d+\] Step \d+ residual norm = \S+$", p.stdout, re.M)
    assert printed == want, "first differing line: %s" % (next((a, b_) for a, b_ in zip(printed + [None], want + [None]) if a != b_),)
    got = re.findall(r"^k = (\S+): converged after (\d+) steps, \|x\|\^2 = (\S+)$", p.stdout, re.M)
    assert [int(m[1]) for m in got] == eo.last_iterations and all(eo.last_converged)
    assert [m[2] for m in got] == ["%.10e" % x.squarednorm() for x in xs]
    assert len(set(eo.last_iterations)) == len(KS)
