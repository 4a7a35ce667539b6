"""step_pair_kernel (csrc/gcr_steppair.hip) runs the one-launch GCR steps of the restart-5 headline — in-cycle steps at 1..4 stored
directions and the close at 5, real coefficients, with the next residual update — as ONE workgroup per CU that carries two of the
512 logical workgroups: a thread owns the 2 x 4 rows the two gave it and keeps all eight rows of Ap_0 (and rows of Ap_1) from the
pass-1 dots to the build.  Every sum keeps its operands, its order and its tree, and the partial sums stay indexed by logical
workgroup, so the default path must give the iteration count, the history and x of the keep forms (option "step_build_pair" = 0)
and of the three-kernel path (option "step_build" = 0) BIT FOR BIT, and the counter "step_pair_launches" must say where the pair
forms ran: the steps of every enabled form (PAIR_IN_CYCLE, PAIR_CLOSE_AT_5: the gate of csrc/gcr_steppair.hip sb_pair_form, pinned
by tests/test_stepbuild_pair_regs.py), none with the option off, none for a DiracOp (complex shift) or another stencil shape.
Shapes: 96 x 96 x 57 (525 312 rows: most threads own one row, the second trip exists in logical workgroup 0 only), 97 x 96 x 57
(the last wave half beyond `end`), 96 x 120 x 112 (threads with 2 and with 3 rows), 128^3 (eight full rows per thread)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from tests.test_gpu_stepbuild_apply_lanes import _shifted_band_op  # noqa: E402
from tests.test_gpu_stepbuild_reuse import _box_op, _same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(96, 96, 57), (97, 96, 57), (96, 120, 112), (128, 128, 128)]
# (restart, max_it) — steps 1 .. max_it - 1 are launches, each with the next residual update: (5, 12) two closes at 5 and an end
# inside a cycle; (5, 9) the solve ends on the 4-direction step; (5, 6) on the step after a close; (5, 10) on a close; (4, 9) and
# (3, 7): cycles whose closes (at 4 and 3 directions) are not pair forms — they take only the in-cycle steps
SETTINGS = [(5, 12), (5, 9), (5, 6), (5, 10), (4, 9), (3, 7)]
# the forms the default dispatch hands out (sb_pair_form)
PAIR_IN_CYCLE = (2, 3, 4)
PAIR_CLOSE_AT_5 = False


def _pair_steps(restart, max_it):
    """launches of step_pair_kernel in a stand-alone solve of max_it steps that does not stop early: step `it` (1-based) holds
    nd = (it - 1) % restart + 1 directions and closes a cycle where nd == restart"""
    n = 0
    for it in range(1, max_it):
        nd = (it - 1) % restart + 1
        n += (nd == 5 and PAIR_CLOSE_AT_5) if nd == restart else nd in PAIR_IN_CYCLE
    return n


def _solve(op, dims, b, restart, max_it, tol, option=None):
    """(x, history, iterations, one-launch step launches, step_pair_kernel launches) of one solve, `option` off for its duration"""
    import mgpreconditionedgcr_amd as mg
    prev = mg.set_option(option, 0) if option else None
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        before, pair = mg.stat("step_build_launches"), mg.stat("step_pair_launches")
        g.solve(b, x)
        return (x.to_numpy().copy(), g.last_history.copy(), g.last_iterations, mg.stat("step_build_launches") - before,
                mg.stat("step_pair_launches") - pair)
    finally:
        if option:
            mg.set_option(option, prev)


def _cases():
    out = []
    for si, dims in enumerate(SHAPES):
        for ci, (restart, max_it) in enumerate(SETTINGS):
            # a DiracOp (1 - k A with a complex k: no pair form is handed out for a shifted operator) once per shape
            out.append(pytest.param(dims, restart, max_it, ci == si, id="%dx%dx%d-r%d-it%d%s" % (*dims, restart, max_it, "-dirac" if ci == si else "")))
    return out


@pytest.mark.parametrize("dims,restart,max_it,dirac", _cases())
def test_pair_bit_for_bit(dims, restart, max_it, dirac):
    import mgpreconditionedgcr_amd as mg
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, restart, max_it, 0.0)
    keep = _solve(op, dims, b, restart, max_it, 0.0, "step_build_pair")
    three = _solve(op, dims, b, restart, max_it, 0.0, "step_build")
    assert new[3] > 0, "the default path did not take the one-launch steps"
    assert three[3] == 0 and keep[3] == new[3], (new[3], three[3], keep[3])
    assert keep[4] == 0 and three[4] == 0, (keep[4], three[4])
    want = 0 if dirac else _pair_steps(restart, max_it)
    assert new[4] == want, (new[4], want)
    assert dirac or want > 0   # (every setting has a step of an enabled form)
    _same(new, keep)
    _same(new, three)
    assert new[2] == max_it and np.all(np.isfinite(new[0]))


def test_pair_needs_the_keep_forms():
    """with "step_build_keep_all" = 0 the dispatch is step_build_kernel's, as before"""
    import mgpreconditionedgcr_amd as mg
    dims = SHAPES[0]
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, 5, 12, 0.0)
    build = _solve(op, dims, b, 5, 12, 0.0, "step_build_keep_all")
    assert build[3] == new[3] > 0 and build[4] == 0, (new[3], build[3], build[4])
    _same(new, build)


@pytest.fixture(scope="module")
def stop_case():
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 96)
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(96)
    h = _solve(op, dims, b, 5, 12, 0.0, "step_build")[1]
    h.setflags(write=False)
    return dims, op, b, h


@pytest.mark.parametrize("stop_at", [4, 10])
def test_pair_device_stop(stop_case, stop_at):
    """the tolerance is met at a 4-direction step (the step decides `ends_here` in both of its logical workgroups and leaves its
    residual update out) and at the close of the second cycle"""
    dims, op, b, h = stop_case
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    new = _solve(op, dims, b, 5, 200, tol)
    keep = _solve(op, dims, b, 5, 200, tol, "step_build_pair")
    three = _solve(op, dims, b, 5, 200, tol, "step_build")
    assert new[2] == stop_at
    assert keep[4] == 0 and three[4] == 0, (keep[4], three[4])
    if PAIR_IN_CYCLE or PAIR_CLOSE_AT_5:
        assert new[4] > 0
    _same(new, keep)
    _same(new, three)


def test_another_middle_dispatches_as_before():
    """the +1 band moved to +2: the stencil's middle slots are not (-1, 0, +1), the keep forms' apply is not handed out and neither
    is the pair form"""
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 57)
    op = _shifted_band_op(dims)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, 5, 12, 0.0)
    three = _solve(op, dims, b, 5, 12, 0.0, "step_build")
    assert new[3] > 0 and three[3] == 0, (new[3], three[3])
    assert new[4] == 0 and three[4] == 0, (new[4], three[4])
    _same(new, three)
