"""The start of a solve as one launch (csrc/gcr_stepbuild.hip start_build_kernel, mgcr_set_option "start_build") and the one-launch
steps that read r once and keep it in registers (step_keep_kernel, "step_build_keep_all"): each switched on and off must give the same
iteration count, history and x bit for bit, and the one-launch start must actually have run where it is eligible."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu

OFF = {"start_build": 0, "step_build_keep_all": 0}


def _problem(n, dirac):
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import problems
    N, ncol, rowptr, col, val = problems.poisson3d_csr(n)
    A = mg.Sparse(N, ncol, rowptr, col, val)
    op = mg.DiracOp(A, 0.05 - 0.02j) if dirac else A
    dims = (n, n, n)
    return op, dims, mg.Field(dims).fill_rhs(n)


def _solve(op, dims, b, restart, max_it, tol, opts):
    import mgpreconditionedgcr_amd as mg
    prev = {k: mg.set_option(k, v) for k, v in opts.items()}
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        before = mg.stat("start_build_launches")
        g.solve(b, x)
        return x.to_numpy().copy(), g.last_history.copy(), g.last_iterations, mg.stat("start_build_launches") - before
    finally:
        for k, v in prev.items():
            mg.set_option(k, v)


def _same(a, b):
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("n,restart,max_it,dirac", [(128, 5, 20, False), (96, 5, 1, False), (96, 5, 4, False), (96, 5, 5, False),
                                                    (96, 5, 6, False), (128, 5, 23, True), (96, 10, 20, False), (96, 3, 8, True)])
def test_parts_on_off_bit_for_bit(n, restart, max_it, dirac):
    op, dims, b = _problem(n, dirac)
    on = _solve(op, dims, b, restart, max_it, 0.0, {})
    off = _solve(op, dims, b, restart, max_it, 0.0, OFF)
    start_off = _solve(op, dims, b, restart, max_it, 0.0, {"start_build": 0})
    keep_off = _solve(op, dims, b, restart, max_it, 0.0, {"step_build_keep_all": 0})
    for other in (off, start_off, keep_off):
        _same(on, other)
    assert off[3] == 0 and start_off[3] == 0
    # restart <= 5: the start is one launch; restart 10: its later closing steps are not, so the start is not either; a solve
    # shorter than a cycle takes the start that reads b as P0 anyway (gcr.hip alias_p0)
    assert on[3] == (1 if restart <= 5 and max_it >= restart else 0), on[3]
    assert on[2] == max_it and np.all(np.isfinite(on[0]))


@pytest.mark.parametrize("stop_at", [3, 6])
def test_device_stop_before_and_after_the_first_close(stop_at):
    """tolerances met at step 3 (the closing step at 5 is enqueued and is a no-op: x must be flushed from P0 = b) and at step 6"""
    op, dims, b = _problem(96, False)
    ref = _solve(op, dims, b, 5, 12, 0.0, OFF)
    h = ref[1]
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    on = _solve(op, dims, b, 5, 200, tol, {})
    off = _solve(op, dims, b, 5, 200, tol, OFF)
    assert on[3] == 1 and on[2] == stop_at
    _same(on, off)
