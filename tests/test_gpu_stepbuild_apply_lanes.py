"""The apply at the head of the one-launch steps that keep r on chip (csrc/gcr_stepbuild_keep_body.h, real stencil coefficients)
takes the row's own r from the stencil's diagonal gather (spmv_dev.h sten_row_product_own_t) instead of loading it a second time
behind the gathers; the host hands these forms out only for a stencil view whose middle slots are (-1, 0, +1) (sten_lane_middle).
(The other half of the change — r[i - 1], r[i + 1] from the neighbouring lanes of the wave, only lane 0's left and lane 63's right
neighbour loaded — passed these tests too and was measured slower: it is not built; the shapes below are the
ones that exercise it and stay.)  Every slot holds the bits the gathers brought, so the default path must give the iteration
count, the history and x of the step_build_kernel dispatch (option "step_build_keep_all" = 0) and of the three-kernel path (option
"step_build" = 0) BIT FOR BIT, and the counter "step_apply_own_launches" must say where the new apply ran.
Shapes: 128^3 (four full trips per thread); 96 x 120 x 112 (threads with 2 and with 3 rows: whole waves beyond `end`); 96 x 96 x 57
(lines of 57: line ends fall inside waves, where the absent +-1 slot of a row meets the neighbouring lane's live value); 97 x 96 x 57
(530 784 rows = 8293 waves and 32 rows: the last wave is partly beyond `end`, and its lanes there enter the row product with
clamped loads).  An operator whose 7-slot stencil view has another middle (the +1 band moved to +2) must take step_build_kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from tests.test_gpu_stepbuild_keep_wide import _box_op, _same, _solve  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 128), (96, 120, 112), (96, 96, 57), (97, 96, 57)]
SETTINGS = [(5, 12), (5, 6), (4, 9), (3, 7)]


def _solve_l(op, dims, b, restart, max_it, option=None):
    """_solve's tuple + the launches whose apply took the own r from the diagonal gather"""
    import mgpreconditionedgcr_amd as mg
    before = mg.stat("step_apply_own_launches")
    out = _solve(op, dims, b, restart, max_it, 0.0, option)
    return out + (mg.stat("step_apply_own_launches") - before,)


def _cases():
    out = []
    for si, dims in enumerate(SHAPES):
        for ci, (restart, max_it) in enumerate(SETTINGS):
            # a DiracOp (complex shift: the row's own r enters A r) once per shape, at another setting each
            out.append(pytest.param(dims, restart, max_it, ci == si, id="%dx%dx%d-r%d-it%d%s" % (*dims, restart, max_it, "-dirac" if ci == si else "")))
    return out


@pytest.mark.parametrize("dims,restart,max_it,dirac", _cases())
def test_apply_own_bit_for_bit(dims, restart, max_it, dirac):
    import mgpreconditionedgcr_amd as mg
    assert 2 ** 19 < dims[0] * dims[1] * dims[2] <= 2 ** 21
    op = _box_op(dims, dirac)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve_l(op, dims, b, restart, max_it)
    build = _solve_l(op, dims, b, restart, max_it, "step_build_keep_all")
    three = _solve_l(op, dims, b, restart, max_it, "step_build")
    assert new[3] > 0, "the default path did not take the one-launch steps"
    assert three[3] == 0 and build[3] == new[3], (new[3], three[3], build[3])
    assert new[5] > 0 and build[5] == 0 and three[5] == 0, (new[5], build[5], three[5])
    _same(new, build)
    _same(new, three)
    assert new[2] == max_it and np.all(np.isfinite(new[0]))


def _shifted_band_op(dims):
    """the box operator with its +1 band moved to +2: seven slots (-ny nx, -nx, -1, 0, +2, +nx, +ny nx), columns ascending in every row"""
    import mgpreconditionedgcr_amd as mg
    nz, ny, nx = dims
    i, j, k = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    r = (i * ny + j) * nx + k
    cand = [(i > 0, r - ny * nx, -1.0), (j > 0, r - nx, -1.0), (k > 0, r - 1, -1.0), (np.ones_like(r, bool), r, 6.0),
            (k < nx - 2, r + 2, -1.0), (j < ny - 1, r + nx, -1.0), (i < nz - 1, r + ny * nx, -1.0)]
    mask = np.stack([c[0] for c in cand], axis=1)
    cols = np.stack([c[1] for c in cand], axis=1)
    vals = np.broadcast_to(np.array([c[2] for c in cand]), mask.shape)
    rowptr = np.zeros(r.size + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=rowptr[1:])
    return mg.Sparse(r.size, r.size, rowptr, cols[mask], vals[mask].astype(np.complex128))


def test_another_middle_takes_step_build_kernel():
    import mgpreconditionedgcr_amd as mg
    dims = (96, 96, 57)
    op = _shifted_band_op(dims)
    b = mg.Field(dims).fill_rhs(dims[0])
    new = _solve_l(op, dims, b, 5, 12)
    three = _solve_l(op, dims, b, 5, 12, "step_build")
    assert new[3] > 0, "the operator did not take the one-launch steps"
    assert three[3] == 0
    assert new[4] == 0 and new[5] == 0 and three[5] == 0, (new[4], new[5], three[5])
    _same(new, three)
    assert new[2] == 12 and np.all(np.isfinite(new[0]))
