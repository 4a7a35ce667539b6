"""LowPrecisionEvenOddGCR of the C++ mirror (include/mgcr/mgcr_dropin.hpp) through examples/mixed_precision_evenodd.cpp: it compiles
with g++, and on the GPU it solves the sample at k = 0.18 through EvenOddDiracOp::solve both ways — the fp64 GCR(5) on the Schur system
alone, and with the fp32 Schur GCR as flexible right preconditioner — to true residuals of the full system below 1e-9 and the same
solution, in the 22 outer steps the numpy model and the Python mirror take."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "build", "mixed_precision_evenodd")


def test_example_compiles_with_gxx():
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_both_solves_agree(sample_matrix_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    d = os.path.dirname(sample_matrix_path)
    p = subprocess.run([EXE, os.path.basename(sample_matrix_path), "0.18"], capture_output=True, text=True,
                       env=dict(os.environ, MGCR_SAMPLE_DIR=d), timeout=300, cwd=d)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.rstrip().endswith("OK")
    assert "fp32 Schur copy: 3072 rows (1536 even, 1536 odd), widths 39 / 39, 0 / 0 tail rows, complex slab, no diagonal" in p.stdout
    plain = int(re.search(r"^even-odd fp64: converged after (\d+) steps$", p.stdout, re.M).group(1))
    mixed = int(re.search(r"^even-odd mixed: converged after (\d+) outer steps", p.stdout, re.M).group(1))
    assert mixed < plain
