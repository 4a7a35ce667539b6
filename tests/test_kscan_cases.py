"""CPU check of the premise of the scan test on the GPU (tests/test_gpu_kscan.py): on the sample operator with rhs_grid(3072, 1),
GCR(5), tol 1e-10 and max_iter 400, the oracle in the reference's summation order stops the six hopping parameters of
tests/kscan_cases.py at five distinct steps, and k = 0.20 runs to max_iter unconverged with a finite residual of about 50."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import kscan_cases as kc


@pytest.fixture(scope="module")
def sample_op(sample_matrix_path):
    nrow, ncol, rowptr, col, val = orc.read_text_csr(sample_matrix_path)
    assert nrow == ncol == 3072
    return orc.csr(nrow, ncol, rowptr, col, val)


@pytest.fixture(scope="module")
def scan(sample_op):
    b = orc.rhs_grid(3072, kc.SCAN_RHS_SEED)
    prm = orc.gcr_param(restart=kc.SCAN_RESTART, max_iter=kc.SCAN_MAX_ITER, tol=kc.SCAN_TOL)
    return [orc.gcr_solve(orc.dirac(sample_op, k), prm, b) for k in kc.SCAN_KS]


@pytest.mark.parametrize("j", range(len(kc.SCAN_KS)))
def test_column_stops_where_the_table_says(scan, j):
    x, hist, it, conv = scan[j]
    assert it == kc.SCAN_STOPS[j], (kc.SCAN_KS[j], it, hist[-2:])
    assert hist.size == it + 1 and np.isfinite(hist).all() and np.isfinite(x).all()
    assert bool(conv) == (it != kc.SCAN_MAX_ITER)
    if conv:
        assert hist[-1] <= kc.SCAN_TOL < hist[-2]


def test_five_distinct_stops_and_one_column_that_never_stops(scan):
    its = [c[2] for c in scan]
    assert len(set(its[:5])) == 5 and max(its[:5]) < kc.SCAN_MAX_ITER
    x, hist, it, conv = scan[5]
    assert it == kc.SCAN_MAX_ITER and not conv
    assert np.isfinite(hist[-1]) and 10.0 < hist[-1] < 250.0, hist[-1]     # "about 50": the solve diverges slowly, it does not blow up
