"""step_keep_wide_kernel (csrc/gcr_stepbuild.hip) takes the one-launch steps at 4 stored directions with the next residual update
(inside a restart-5 cycle, and the close of a restart-4 one) and the close at 5, reading r once: step_keep_kernel's body one trip at
a time, without a kept Ap_0 row, at 5 with the trips' offsets formed on the fly.  No element sees another operation or another order, so the default path must give the
iteration count, the history and x of the step_build_kernel dispatch (option "step_build_keep_all" = 0) and of the three-kernel path
(option "step_build" = 0) BIT FOR BIT, and the counter "step_keep_wide_launches" must say where the new entries ran.
Shapes: 128^3 (four full trips per thread), 96 x 120 x 112 (threads with 2 and with 3 rows: the one-trip batches meet a trip beyond
`end`), 96 x 96 x 57 (525 312 rows, just above the 2^19 bound: most threads own one row)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from tests.test_gpu_stepbuild_reuse import _box_op, _same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 128), (96, 120, 112), (96, 96, 57)]
# (restart, max_it) — a solve's last step is bookkeeping only (gcr.hip step_finish), steps 1 .. max_it - 1 are launches: (5, 12) two
# closes at 5 and an end inside a cycle; (5, 9) the solve ends on the 4-direction step; (5, 6) on the step after a close; (5, 10)
# on a close (steps 9 and 10 of a stand-alone solve: the last launch is the 4-direction step, the close itself launches nothing);
# (4, 9): the closes at 4 directions are the new entries' only steps; (3, 7): cycles in which they have none
SETTINGS = [(5, 12), (5, 9), (5, 6), (5, 10), (4, 9), (3, 7)]


def _wide_steps(restart, max_it):
    """launches of step_keep_wide_kernel in a stand-alone solve of max_it steps that does not stop early: step `it` (1-based) holds
    nd = (it - 1) % restart + 1 directions and closes a cycle where nd == restart; the steps before the last are launches, each with
    the next step's residual update"""
    return sum((it - 1) % restart + 1 >= 4 for it in range(1, max_it))


def _solve(op, dims, b, restart, max_it, tol, option=None):
    """(x, history, iterations, one-launch step launches, step_keep_wide_kernel launches) of one solve, `option` off for its duration"""
    import mgpreconditionedgcr_amd as mg
    prev = mg.set_option(option, 0) if option else None
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        before, wide = mg.stat("step_build_launches"), mg.stat("step_keep_wide_launches")
        g.solve(b, x)
        return (x.to_numpy().copy(), g.last_history.copy(), g.last_iterations, mg.stat("step_build_launches") - before,
                mg.stat("step_keep_wide_launches") - wide)
    finally:
        if option:
            mg.set_option(option, prev)


def _cases():
    out = []
    for si, dims in enumerate(SHAPES):
        for ci, (restart, max_it) in enumerate(SETTINGS):
            # a DiracOp (complex shift: the complex-coefficient entries) once per shape, at a restart-5 setting, another one each
            out.append(pytest.param(dims, restart, max_it, ci == si, id="%dx%dx%d-r%d-it%d%s" % (*dims, restart, max_it, "-dirac" if ci == si else "")))
    return out


@pytest.mark.parametrize("dims,restart,max_it,dirac", _cases())
def test_keep_wide_bit_for_bit(dims, restart, max_it, dirac):
    import mgpreconditionedgcr_amd as mg
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, restart, max_it, 0.0)
    build = _solve(op, dims, b, restart, max_it, 0.0, "step_build_keep_all")
    three = _solve(op, dims, b, restart, max_it, 0.0, "step_build")
    assert new[3] > 0, "the default path did not take the one-launch steps"
    assert three[3] == 0 and build[3] == new[3], (new[3], three[3], build[3])
    assert build[4] == 0 and three[4] == 0, (build[4], three[4])
    assert new[4] == _wide_steps(restart, max_it), (new[4], _wide_steps(restart, max_it))
    if restart == 5 and max_it >= 6:
        assert new[4] > 0
    _same(new, build)
    _same(new, three)
    assert new[2] == max_it and np.all(np.isfinite(new[0]))


@pytest.fixture(scope="module")
def stop_case():
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 96)
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(96)
    h = _solve(op, dims, b, 5, 12, 0.0, "step_build")[1]
    h.setflags(write=False)
    return dims, op, b, h


@pytest.mark.parametrize("stop_at", [4, 9, 10])
def test_keep_wide_device_stop(stop_case, stop_at):
    """the tolerance is met at a 4-direction step (4, 9: the step decides `ends_here` and leaves its residual update out) and at
    the close of the second cycle (10: the close decides it)"""
    dims, op, b, h = stop_case
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    new = _solve(op, dims, b, 5, 200, tol)
    build = _solve(op, dims, b, 5, 200, tol, "step_build_keep_all")
    three = _solve(op, dims, b, 5, 200, tol, "step_build")
    assert new[2] == stop_at
    assert new[4] > 0 and build[4] == 0 and three[4] == 0, (new[4], build[4], three[4])
    _same(new, build)
    _same(new, three)


_NO_XR_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import mgpreconditionedgcr_amd as mg
from tests.test_gpu_stepbuild_keep_wide import _box_op, _same, _solve
mg.init(0)
dims = (96, 120, 112)
for dirac in (False, True):
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, 5, 12, 0.0)
    build = _solve(op, dims, b, 5, 12, 0.0, "step_build_keep_all")
    three = _solve(op, dims, b, 5, 12, 0.0, "step_build")
    _same(new, build)
    _same(new, three)
    # the closes at 5 (steps 5 and 10, no update behind them) take the new entry; steps 4 and 9 (4 directions) step_build_kernel
    assert new[3] == build[3] > 0 and three[3] == 0, (new[3], build[3], three[3])
    assert new[4] == 2 and build[4] == 0 and three[4] == 0, (new[4], build[4], three[4])
    assert new[2] == 12 and np.all(np.isfinite(new[0]))
print("no-xr OK")
"""


def test_keep_wide_without_the_residual_update():
    """MGCR_STEPBUILD_XR=0 (read once per process, hence a child): no launch carries the next residual update — the form a nested
    solve's last close takes.  The closes at 5 run step_keep_wide_kernel<5, false, true, *>, and the 4-direction steps, whose form
    without the update is not built (measured no faster), fall back to step_build_kernel — the same bits"""
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, MGCR_STEPBUILD_XR="0")
    p = subprocess.run([sys.executable, "-c", _NO_XR_CHILD % root], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "no-xr OK" in p.stdout, p.stdout + p.stderr
