"""The keep body of the one-launch GCR steps (csrc/gcr_stepbuild_keep_body.h) fetches the operands of the scalar stage behind
exchange 1 (|r|^2 partials, den[], at the close lc->cx and the coefficient table's columns) behind the apply, folds |r|^2 and decides
`ends_here` ahead of the poll, and keeps more rows of Ap_0 in registers from the pass-1 dots to the build (sb_kept_rows; now also
in step_keep_wide_kernel).  The fold is fold_partials' tree, the kept rows hold the values the re-read would fetch: no operation,
operand or order changes, so the default path must give the iteration count, the history and x of the three-kernel path (option
"step_build" = 0) and of the step_build_kernel dispatch (option "step_build_keep_all" = 0) BIT FOR BIT, and the counters
"step_keep_wide_launches" and "step_apply_own_launches" must say that the forms still dispatch as before.
Shapes: 96 x 96 x 57 (525 312 rows: line ends inside waves); 97 x 96 x 57 (530 784 rows: the last wave is half beyond `end`, the
threads own fewer rows than a form keeps: a kept trip beyond `end`); 128^3 (every thread has exactly 4 rows: every kept row used).
A solve that stops on the device — at a cycle's closing step and inside a cycle, the host never looking (check_every beyond the
solve) — is where an `ends_here` decided in the wrong place would show."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from tests.test_gpu_stepbuild_reuse import _box_op, _same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(96, 96, 57), (97, 96, 57), (128, 128, 128)]
# (restart, max_it): two closes at 5 and a last launch without the next residual update; the close at 4 directions; the close at 3
# with the update (step_build_kernel's) between keep steps; the close at 2
SETTINGS = [(5, 12), (4, 9), (3, 7), (2, 5)]


def _expected_launches(restart, max_it, real):
    """(one-launch steps, step_keep_wide_kernel's, those whose apply takes the own r from the diagonal gather) of a stand-alone
    solve that does not stop early, as the commit before dispatched them: step `it` holds nd = (it - 1) % restart + 1 directions and
    closes the cycle where nd == restart; steps 1 .. max_it - 1 are launches, each with the next residual update; step_keep_kernel
    up to 3 directions except the close at 3, step_keep_wide_kernel from 4; the own-r apply in both, for real stencil coefficients
    (a DiracOp's complex shift leaves them real)"""
    nds = [(it - 1) % restart + 1 for it in range(1, max_it)]
    wide = sum(nd >= 4 for nd in nds)
    keep = sum(nd <= 2 or (nd == 3 and restart != 3) for nd in nds)
    return len(nds), wide, (keep + wide) if real else 0


_OPS = {}


def _op(dims, kind):
    """the operator and right-hand side of a shape, built once.  kind: "real" the box Laplacian; "dirac" a DiracOp of it with a
    complex shift (the stencil's coefficients stay real: the forms for real coefficients, the row's own r entering A r);
    "complex" the box Laplacian times 1 + 0.25i (complex stencil coefficients: the REALC = false forms)"""
    import mgpreconditionedgcr_amd as mg
    from mgpreconditionedgcr_amd import problems
    if (dims, kind) not in _OPS:
        if kind == "complex":
            N, ncol, rowptr, col, val = problems.poisson3d_box_csr(*dims)
            op = mg.Sparse(N, ncol, rowptr, col, np.asarray(val, np.complex128) * (1.0 + 0.25j))
        else:
            op = _box_op(dims, kind == "dirac")
        _OPS[(dims, kind)] = (op, mg.Field(dims).fill_rhs(dims[0]))
    return _OPS[(dims, kind)]


def _solve(op, dims, b, restart, max_it, tol, option=None, check_every=0):
    """(x, history, iterations, one-launch steps, step_keep_wide_kernel launches, own-r applies) of one solve, `option` off for it"""
    import mgpreconditionedgcr_amd as mg
    prev = mg.set_option(option, 0) if option else None
    try:
        g = mg.GCR(op, mg.GCR_Param(0, restart, max_it, tol, False, check_every=check_every))
        x = mg.Field(dims).set_zero()
        names = ("step_build_launches", "step_keep_wide_launches", "step_apply_own_launches")
        before = [mg.stat(n) for n in names]
        g.solve(b, x)
        return (x.to_numpy().copy(), g.last_history.copy(), g.last_iterations) + tuple(mg.stat(n) - v for n, v in zip(names, before))
    finally:
        if option:
            mg.set_option(option, prev)


def _cases():
    out = []
    for si, dims in enumerate(SHAPES):
        for ci, (restart, max_it) in enumerate(SETTINGS):
            # once per shape, at another setting each: a DiracOp (complex shift), and complex coefficients (the REALC = false forms)
            kind = "dirac" if ci == si else "complex" if ci == (si + 1) % len(SETTINGS) else "real"
            out.append(pytest.param(dims, restart, max_it, kind, id="%dx%dx%d-r%d-it%d-%s" % (*dims, restart, max_it, kind)))
    return out


@pytest.mark.parametrize("dims,restart,max_it,kind", _cases())
def test_scalar_stage_bit_for_bit(dims, restart, max_it, kind):
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op, b = _op(dims, kind)
    new = _solve(op, dims, b, restart, max_it, 0.0)
    three = _solve(op, dims, b, restart, max_it, 0.0, "step_build")
    build = _solve(op, dims, b, restart, max_it, 0.0, "step_build_keep_all")
    print("launches (one-launch, wide, own-r): default", new[3:], "three-kernel", three[3:], "step_build_kernel", build[3:],
          "expected", _expected_launches(restart, max_it, kind != "complex"))
    assert new[3:] == _expected_launches(restart, max_it, kind != "complex"), new[3:]
    assert three[3:] == (0, 0, 0) and build[3:] == (new[3], 0, 0), (three[3:], build[3:])
    _same(new, three)
    _same(new, build)
    assert new[2] == max_it and np.all(np.isfinite(new[0]))


@pytest.fixture(scope="module")
def stop_case():
    dims = (96, 96, 57)
    op, b = _op(dims, "real")
    h = _solve(op, dims, b, 5, 12, 0.0, "step_build")[1]
    h.setflags(write=False)
    return dims, op, b, h


@pytest.mark.parametrize("stop_at", [5, 10, 7])
def test_scalar_stage_device_stop(stop_case, stop_at):
    """the tolerance, taken from the three-kernel path's history, is met at a cycle's closing step (5, 10: the close decides
    `ends_here` and leaves its residual update out) and inside a cycle (7); the host does not look at the residual before the end"""
    dims, op, b, h = stop_case
    assert h[stop_at] < h[stop_at - 1]
    tol = float(h[stop_at]) * (1 + 1e-9)
    new = _solve(op, dims, b, 5, 40, tol, check_every=1000)
    three = _solve(op, dims, b, 5, 40, tol, "step_build", check_every=1000)
    print("stop at", stop_at, "iterations", new[2], three[2], "history lengths", len(new[1]), len(three[1]), "launches", new[3:])
    assert new[2] == three[2] == stop_at, (new[2], three[2])
    assert len(new[1]) == len(three[1])
    assert new[3] > 0 and three[3] == 0
    _same(new, three)
