"""step_pair_late_kernel (csrc/gcr_steppair_late.hip) is step_pair_kernel's body (csrc/gcr_steppair_body.h) under the policy that
does not hold r of the thread's eight rows from the apply to the build: the apply drops the own value of its diagonal gather, the
build loads the element again from the same vector — which nothing writes during the launch — and 8 to 9 thread-rows of the stored
directions more stay in registers across exchange 1.  Same operands, same order, same trees: with option "step_build_pair_late" = 2
(every built form: 3 and 4 directions in a cycle, the close at 5) and = 1 (the forms handed out by default, sb_pair_late_form,
pinned by tests/test_stepbuild_pair_late_regs.py) the iteration count, the history and x must be BIT FOR BIT those of
  * "step_build_pair_late" = 0 (step_pair_kernel),   * "step_build_pair" = 0 (the keep forms),
  * "step_build" = 0 (three kernels),                * "step_build_keep_all" = 0 (step_build_kernel).
The counter "step_pair_late_launches" says where the new kernel ran: the steps of the forms in force, none with option 0, with the
pair option off, for a DiracOp (complex shift) or another stencil shape; "step_pair_launches" keeps the values of
tests/test_gpu_stepbuild_pair.py (a step at 2..4 directions, whichever pair kernel ran it; not the close).
Shapes (tests/test_gpu_stepbuild_pair.py): 96 x 96 x 57 (the second trip exists in logical workgroup 0 only), 97 x 96 x 57 (the
last wave half beyond `end`), 96 x 120 x 112 (threads with 2 and with 3 rows), 128^3 (eight full rows per thread)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from tests.test_gpu_stepbuild_apply_lanes import _shifted_band_op  # noqa: E402
from tests.test_gpu_stepbuild_pair import SETTINGS, SHAPES, _pair_steps  # noqa: E402
from tests.test_gpu_stepbuild_reuse import _box_op, _same  # noqa: E402

pytestmark = pytest.mark.gpu

# the built late forms (option 2) and the ones the default dispatch hands out (option 1, sb_pair_late_form)
BUILT_IN_CYCLE, BUILT_CLOSE_AT_5 = (3, 4), True
GATE_IN_CYCLE, GATE_CLOSE_AT_5 = (3, 4), True
REFERENCES = ("step_build_pair_late", "step_build_pair", "step_build", "step_build_keep_all")


def _late_steps(restart, max_it, mode):
    """launches of step_pair_late_kernel in a stand-alone solve of max_it steps that does not stop early (see _pair_steps)"""
    in_cycle, close5 = {0: ((), False), 1: (GATE_IN_CYCLE, GATE_CLOSE_AT_5), 2: (BUILT_IN_CYCLE, BUILT_CLOSE_AT_5)}[mode]
    n = 0
    for it in range(1, max_it):
        nd = (it - 1) % restart + 1
        n += (nd == 5 and close5) if nd == restart else nd in in_cycle
    return n


def _solve(op, dims, b, restart, max_it, tol, mode, off=None):
    """(x, history, iterations, one-launch steps, pair steps, step_pair_late_kernel launches) of one solve with
    "step_build_pair_late" = mode and option `off` switched off for its duration"""
    import mgpreconditionedgcr_amd as mg
    prev_mode = mg.set_option("step_build_pair_late", mode)
    prev = mg.set_option(off, 0) if off else None
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False))
        x = mg.Field(dims).set_zero()
        names = ("step_build_launches", "step_pair_launches", "step_pair_late_launches")
        before = [mg.stat(n) for n in names]
        g.solve(b, x)
        return (x.to_numpy().copy(), g.last_history.copy(), g.last_iterations) + tuple(mg.stat(n) - v for n, v in zip(names, before))
    finally:
        if off:
            mg.set_option(off, prev)
        mg.set_option("step_build_pair_late", prev_mode)


def _references(op, dims, b, restart, max_it, tol):
    """the four references: option 0, the pair option off, three kernels, step_build_kernel — none launches the new kernel"""
    refs = []
    for off in REFERENCES:
        r = _solve(op, dims, b, restart, max_it, tol, 0 if off == "step_build_pair_late" else 2, None if off == "step_build_pair_late" else off)
        assert r[5] == 0, (off, r[5])
        refs.append(r)
    return refs


@pytest.mark.parametrize("restart,max_it", SETTINGS, ids=["r%d-it%d" % s for s in SETTINGS])
@pytest.mark.parametrize("dims", SHAPES, ids=["%dx%dx%d" % d for d in SHAPES])
def test_pair_late_bit_for_bit(dims, restart, max_it):
    import mgpreconditionedgcr_amd as mg
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(dims[0])
    zero, keep, three, build = _references(op, dims, b, restart, max_it, 0.0)
    assert zero[5] == 0 and keep[5] == 0 and three[5] == 0 and build[5] == 0, (zero[5], keep[5], three[5], build[5])
    assert zero[4] == _pair_steps(restart, max_it) and keep[4] == 0 and three[4] == 0, (zero[4], keep[4], three[4])
    assert three[3] == 0 and zero[3] == keep[3] == build[3] > 0, (zero[3], keep[3], three[3], build[3])
    for mode in (2, 1):
        new = _solve(op, dims, b, restart, max_it, 0.0, mode)
        print(dims, restart, max_it, "option", mode, "late launches", new[5], "pair steps", new[4], "one-launch steps", new[3])
        assert new[5] == _late_steps(restart, max_it, mode), (mode, new[5], _late_steps(restart, max_it, mode))
        assert new[4] == _pair_steps(restart, max_it), (mode, new[4], _pair_steps(restart, max_it))
        assert new[3] == zero[3], (new[3], zero[3])
        for ref in (zero, keep, three, build):
            _same(new, ref)
        assert new[2] == max_it and np.all(np.isfinite(new[0]))
    assert _late_steps(restart, max_it, 2) > 0 or restart == 3   # (restart 3 has no step of a built late form)


@pytest.mark.parametrize("mode", [2, 1])
def test_no_late_form_for_a_shifted_operator(mode):
    """a DiracOp (1 - k A with a complex k) keeps the keep forms: neither pair kernel runs"""
    import mgpreconditionedgcr_amd as mg
    dims = SHAPES[0]
    op = _box_op(dims, True)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, 5, 12, 0.0, mode)
    three = _solve(op, dims, b, 5, 12, 0.0, mode, "step_build")
    assert new[3] > 0 and new[4] == 0 and new[5] == 0, new[3:]
    _same(new, three)


@pytest.mark.parametrize("mode", [2, 1])
def test_no_late_form_for_another_middle(mode):
    """the +1 band moved to +2: the keep forms' apply is not handed out, and neither pair form is"""
    import mgpreconditionedgcr_amd as mg
    dims = SHAPES[0]
    op = _shifted_band_op(dims)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve(op, dims, b, 5, 12, 0.0, mode)
    three = _solve(op, dims, b, 5, 12, 0.0, mode, "step_build")
    assert new[3] > 0 and new[4] == 0 and new[5] == 0, new[3:]
    _same(new, three)


@pytest.fixture(scope="module")
def stop_case():
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 96)
    op = _box_op(dims, False)
    b = mg.Field(dims).fill_rhs(96)
    h = _solve(op, dims, b, 5, 12, 0.0, 0, "step_build")[1]
    h.setflags(write=False)
    return dims, op, b, h


@pytest.mark.parametrize("stop_at", [4, 10])
def test_pair_late_device_stop(stop_case, stop_at):
    """the tolerance is met at a 4-direction step (the step decides `ends_here` in both of its logical workgroups and leaves its
    residual update out: r, loaded again in the build, is not used after it) and at the close of the second cycle"""
    dims, op, b, h = stop_case
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    refs = _references(op, dims, b, 5, 200, tol)
    for mode in (2, 1):
        new = _solve(op, dims, b, 5, 200, tol, mode)
        assert new[2] == stop_at
        # (the host may have queued steps beyond the stop, which return at once: no exact count here)
        if mode == 2 or GATE_IN_CYCLE or GATE_CLOSE_AT_5:
            assert new[5] > 0
        for ref in refs:
            _same(new, ref)
