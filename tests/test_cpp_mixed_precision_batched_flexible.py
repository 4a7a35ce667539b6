"""GCR::solve_multi with a flexible right preconditioner through the C++ mirror (include/mgcr/mgcr_dropin.hpp) and
examples/mixed_precision_batched_flexible.cpp: it compiles with g++, and on the GPU it solves the sample at k = 0.18 for a block of 4
right-hand sides by one batched GCR(5) around the k-wide fp32 inner solve — every column converged, true residuals below 1e-9, the
step count and the x of the single mixed solve of that column (the example's own exit status) — beside the defect correction."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "build", "mixed_precision_batched_flexible")


def test_example_compiles_with_gxx():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_every_column_has_the_single_mixed_solves_steps_and_solution(sample_matrix_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    d = os.path.dirname(sample_matrix_path)
    p = subprocess.run([EXE, os.path.basename(sample_matrix_path), "0.18"], capture_output=True, text=True,
                       env=dict(os.environ, MGCR_SAMPLE_DIR=d), timeout=300, cwd=d)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.rstrip().endswith("OK")
    cols = re.findall(r"^column (\d): flexible batched GCR converged after (\d+) outer steps \(single mixed solve: (\d+), defect correction: (\d+)\), "
                      r"true residual ([0-9.e+-]+),", p.stdout, re.M)
    assert [int(c[0]) for c in cols] == [0, 1, 2, 3], p.stdout
    for _, steps, single, defect, res in cols:
        assert 1 <= int(steps) == int(single) <= 400 and int(defect) >= 1 and float(res) <= 1e-9, p.stdout
