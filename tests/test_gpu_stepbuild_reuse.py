"""One-launch GCR steps that reuse what they hold (csrc/gcr_stepbuild.hip): step_keep_kernel takes the build's first Ap_0 rows
from the registers of its pass-1 dots, and the closing step_build_kernel at 4 and 5 stored directions runs its close pass and its
build as one loop over the rows, the thread's last close row behind the exchange-2 publish.  Neither changes an operation or an
order of operations on any element, so the default path must give the iteration count, the history and x of the three-kernel path
(option "step_build" = 0) and of the step_build_kernel dispatch (option "step_build_keep_all" = 0) BIT FOR BIT.
Shapes: 128^3 (four full trips per thread: every kept row used, the last row is trip 3), 96 x 120 x 112 (threads with 2 and with 3
rows: a kept trip beyond `end`, the last-row index differs inside a workgroup), 96 x 96 x 57 (525 312 rows, just above the 2^19
bound: workgroup 0's threads own 2 rows, all others 1 — fewer rows than the kept trips)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 128), (96, 120, 112), (96, 96, 57)]
# (restart, max_it): two closes with the next residual update and an end inside a cycle; the 4-direction close; short cycles;
# (5, 10): the solve's last step is a close WITHOUT a residual update behind it
SETTINGS = [(5, 12), (4, 9), (2, 5), (5, 10)]


def _box_op(dims, dirac):
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import problems
    N, ncol, rowptr, col, val = problems.poisson3d_box_csr(*dims)
    A = mg.Sparse(N, ncol, rowptr, col, val)
    return mg.DiracOp(A, 0.05 - 0.02j) if dirac else A


def _solve(op, dims, b, restart, max_it, tol, option=None):
    """(x, history, iterations, one-launch step launches) of one solve, with `option` switched off for its duration"""
    import mgpreconditionedgcr_amd as mg
    prev = mg.set_option(option, 0) if option else None
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        before = mg.stat("step_build_launches")
        g.solve(b, x)
        return x.to_numpy().copy(), g.last_history.copy(), g.last_iterations, mg.stat("step_build_launches") - before
    finally:
        if option:
            mg.set_option(option, prev)


def _same(a, b):
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], b[0])


def _cases():
    out = []
    for si, dims in enumerate(SHAPES):
        for ci, (restart, max_it) in enumerate(SETTINGS):
            # a DiracOp (complex shift: the REALC = false kernels) once per shape, at a different setting each
            out.append(pytest.param(dims, restart, max_it, ci == si, id="%dx%dx%d-r%d-it%d%s" % (*dims, restart, max_it, "-dirac" if ci == si else "")))
    return out


@pytest.mark.parametrize("dims,restart,max_it,dirac", _cases())
def test_reuse_bit_for_bit(dims, restart, max_it, dirac):
    import mgpreconditionedgcr_amd as mg
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, restart, max_it, 0.0)
    three = _solve(op, dims, b, restart, max_it, 0.0, "step_build")
    build = _solve(op, dims, b, restart, max_it, 0.0, "step_build_keep_all")
    assert new[3] > 0, "the default path did not take the one-launch steps"
    assert three[3] == 0 and build[3] == new[3], (new[3], three[3], build[3])
    _same(new, three)
    _same(new, build)
    assert new[2] == max_it and np.all(np.isfinite(new[0]))


def test_reuse_device_stop_at_a_close():
    """the tolerance is met at step 5, the step that closes the first cycle (the merged closing loop, then a no-op update)"""
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 96)
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(96)
    h = _solve(op, dims, b, 5, 12, 0.0, "step_build")[1]
    assert h[5] < h[4]
    tol = float(h[5]) * (1 + 1e-9)
    new = _solve(op, dims, b, 5, 200, tol)
    three = _solve(op, dims, b, 5, 200, tol, "step_build")
    build = _solve(op, dims, b, 5, 200, tol, "step_build_keep_all")
    assert new[2] == 5 and new[3] > 0
    _same(new, three)
    _same(new, build)
