"""One-launch GCR steps that read r once and keep it in registers (csrc/gcr_stepbuild.hip step_keep_kernel, option
"step_build_keep_all") against the step_build_kernel dispatch they replace: the same solve must give the same iteration count,
history and x bit for bit — inside cycles and at the closes of every length (restart 2..5), Poisson and DiracOp, a cube and a box
that is not one, stops on the device inside a cycle and at a close."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu


def _box_op(dims, dirac):
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import problems
    N, ncol, rowptr, col, val = problems.poisson3d_box_csr(*dims)
    A = mg.Sparse(N, ncol, rowptr, col, val)
    return mg.DiracOp(A, 0.05 - 0.02j) if dirac else A


def _solve(op, dims, b, restart, max_it, tol, keep_all):
    import mgpreconditionedgcr_amd as mg
    prev = mg.set_option("step_build_keep_all", 1 if keep_all else 0)
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        before = mg.stat("step_build_launches")
        g.solve(b, x)
        return x.to_numpy().copy(), g.last_history.copy(), g.last_iterations, mg.stat("step_build_launches") - before
    finally:
        mg.set_option("step_build_keep_all", prev)


def _same(a, b):
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("dims,restart,max_it,dirac", [((128, 128, 128), 5, 23, False), ((128, 128, 128), 4, 13, True),
                                                       ((96, 120, 112), 2, 9, False), ((96, 120, 112), 3, 11, True),
                                                       ((96, 120, 112), 5, 17, False), ((128, 128, 128), 3, 10, False)])
def test_keep_all_on_off_bit_for_bit(dims, restart, max_it, dirac):
    import mgpreconditionedgcr_amd as mg
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    on = _solve(op, dims, b, restart, max_it, 0.0, True)
    off = _solve(op, dims, b, restart, max_it, 0.0, False)
    _same(on, off)
    assert on[3] > 0 and on[3] == off[3], (on[3], off[3])
    assert on[2] == max_it and np.all(np.isfinite(on[0]))


@pytest.mark.parametrize("stop_at", [3, 5, 8])
def test_keep_all_device_stop(stop_at):
    """tolerance met inside a cycle (3, 8) and at the step that closes one (5)"""
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 96)
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(96)
    h = _solve(op, dims, b, 5, 12, 0.0, False)[1]
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    on = _solve(op, dims, b, 5, 200, tol, True)
    off = _solve(op, dims, b, 5, 200, tol, False)
    assert on[2] == stop_at
    _same(on, off)

