"""The batched GCR (mgcr_gcr_solve_multi, csrc/gcr_multi.hip) against the CPU oracle in the batched solve's summation order, at its cycle,
column-group, freezing and x0 edges.  The cases and the oracle's model are in tests/multi_rhs_cases.py; tests/test_multi_rhs_cases.py checks
their premises on the CPU.  Per column, history, iteration count, convergence flag and x must be np.array_equal to `oracle_columns` — and to
the single solve wherever include/mgcr.h promises that (xr_fuse_kind 0 or 1, more rows than the small-solve limit).

Left out: the rare-tail stencil layout — on one GPU it is reachable through an environment variable only (tests/test_gpu_parity.py
test_rare_tail_stencil_kernels_same_bits); its real form belongs to distributed row blocks, which the batched solve does not take.
Block-CSR row sums are outside the oracle's model: that case is held to the single solve's bits, and to the oracle within the reordering
sensitivity of its own dot products (tests/test_gpu_parity.py hist_close)."""
import os

import numpy as np
import pytest

import mgpreconditionedgcr_amd as mg
from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, HierarchicalSparse, MgcrError, MultiField, Sparse
from oracle import oracle as orc
from tests import multi_rhs_cases as mc
from tests.test_gpu_parity import hist_close

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
SMALL_DEFAULT = int(os.environ.get("MGCR_SMALL_SOLVE_ROWS", "1024"))     # (the library has no getter, see tests/test_gpu_multi_rhs.py)
_OPS, _SINGLE = {}, {}


def by_group(group):
    cs = [c for c in CASES if c.group == group]
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


def device_operator(case):
    """The case's operator on the device (built once per system and option set), with the layout premise of the oracle's model asserted."""
    key = (case.spec, case.shift, case.options)
    if key in _OPS:
        return _OPS[key]
    s = mc.system(case.spec)
    if s.kind == "bcsr":
        A = HierarchicalSparse(s.nb, s.nb, s.rowptr, s.col, s.blocks)
    else:
        prev = [(name, mg.set_option(name, value)) for name, value in case.options]
        try:
            A = Sparse(s.N, s.N, s.rowptr, s.col, s.val)
        finally:
            for name, value in prev:
                mg.set_option(name, value)
        lay, want = A.ell_layout(), mc.host_layout(case.spec)
        assert (lay["ell_width"], lay["lanes"], lay["tail_rows"], lay["tail_chunk_cap"]) == \
               (want["ell_width"], want["lanes"], want["tail_rows"], want["tail_chunk_cap"]), (lay, want)
        assert orc.row_map(s.N, lay["reach"]) == orc.row_map(s.N, want["reach"]), (lay, want)
        assert orc.row_map_plane(s.N, lay["reach"]) == orc.row_map_plane(s.N, want["reach"])
        if case.shift is not None:
            A = DiracOp(A, case.shift)
    _OPS[key] = A
    return A


def fields(case, specs):
    n = mc.system(case.spec).N
    return [Field((n,), mc.column(case.spec, c)) for c in specs]


def solve_multi(case, A, gcr=None):
    """-> [(x, history, iterations, converged)] per column, like mc.oracle_columns"""
    n, k = mc.system(case.spec).N, len(case.rhs)
    prm = GCR_Param(0, case.restart, case.max_iter, case.tol, False, use_x0=case.use_x0, check_every=case.check_every)
    if gcr is None:
        gcr = GCR(A, prm)
    else:
        gcr.param = prm        # read at solve time
    X = MultiField.from_fields(fields(case, case.x0)) if case.x0 is not None else MultiField((n,), k).set_zero()
    before = mg.stat("multi_solves")
    gcr.solve_multi(MultiField.from_fields(fields(case, case.rhs)), X)
    assert mg.stat("multi_solves") == before + 1
    Xh = X.to_numpy()
    return [(Xh[j], gcr.last_history[j], gcr.last_iterations[j], gcr.last_converged[j]) for j in range(k)]


def solve_single(case, A, j):
    key = (case.spec, case.shift, case.options, case.restart, case.max_iter, case.tol, case.rhs[j], case.x0[j] if case.x0 is not None else None)
    if key not in _SINGLE:
        n = mc.system(case.spec).N
        x = fields(case, [case.x0[j]])[0] if case.x0 is not None else Field((n,)).set_zero()
        g = GCR(A, GCR_Param(0, case.restart, case.max_iter, case.tol, False, use_x0=case.use_x0))
        if case.single == "small0":
            mg.lib().mgcr_set_small_solve_rows(0)
        try:
            s0 = mg.stat("small_solves")
            g.solve(fields(case, [case.rhs[j]])[0], x)
            assert mg.stat("small_solves") == s0          # not the one-workgroup path, which sums in another order
        finally:
            mg.lib().mgcr_set_small_solve_rows(SMALL_DEFAULT)
        _SINGLE[key] = (x.to_numpy(), g.last_history, g.last_iterations, g.last_converged)
    return _SINGLE[key]


def assert_same(what, got, ref, nan=False):
    x, h, it, conv = got
    xr, hr, itr, convr = ref
    assert it == itr, "%s: %d iterations against %d" % (what, it, itr)
    assert conv == convr, what
    assert np.array_equal(h, hr, equal_nan=nan), "%s: history differs first at step %d: %r against %r" % (what, int(np.argmax(h != hr)), h, hr)
    assert np.array_equal(x, xr, equal_nan=nan), "%s: x differs in %d of %d entries (max %.3e)" % (what, int((x != xr).sum()), x.size, np.abs(x - xr).max())


def check_case(case, gcr=None):
    A = device_operator(case)
    got = solve_multi(case, A, gcr)
    ref = mc.oracle_columns(case)
    rule = case.single is not None
    if case.single == "rule":          # the premise of include/mgcr.h's bit-for-bit rule
        assert mc.system(case.spec).N > SMALL_DEFAULT
        if not isinstance(A, HierarchicalSparse):
            assert A.xr_fuse_kind() in (0, 1)
    for j in range(len(case.rhs)):
        zero = case.rhs[j] == ("zero",)     # 0 / 0: NaN history and x in the oracle, the single solve and this column alike
        what = "%s column %d" % (case.id, j)
        if case.bits:
            assert_same(what + " against the oracle", got[j], ref[j], nan=zero)
        if rule:
            assert_same(what + " against the single solve", got[j], solve_single(case, A, j), nan=zero)
        if not zero:
            assert np.isfinite(got[j][0]).all() and np.isfinite(got[j][1]).all(), what
    return got


# ---- a. cycles --------------------------------------------------------------------------------------------------------------------
@by_group("cycles")
def test_cycles(case):
    """storage = max_iter + 1 < restart, the last step on / after a closing step, restart 1 (every step closes), the full coefficient table,
    restart > 16 in a short solve; column groups of 1, 2, 4 and a ragged 4; 4 workgroups and a ragged fifth"""
    got = check_case(case)
    if case.expect == "converges":
        assert max(g[2] for g in got) < case.max_iter and all(g[3] for g in got)


@pytest.mark.parametrize("restart,max_iter", mc.UNSUPPORTED)
def test_cycles_longer_than_the_lean_table_are_refused(restart, max_iter):
    case = mc._case("unsupported", "cycles", mc.P16, restart, max_iter, 0.0, mc.grid_cols(3))
    A = device_operator(case)
    n = mc.system(case.spec).N
    X = MultiField((n,), 3).set_zero()
    with pytest.raises(MgcrError) as e:
        GCR(A, GCR_Param(0, restart, max_iter, 0.0, False)).solve_multi(MultiField.from_fields(fields(case, case.rhs)), X)
    assert e.value.code == 7
    assert not X.to_numpy().any()


# ---- b. freezing ------------------------------------------------------------------------------------------------------------------
@by_group("freeze")
def test_freezing(case):
    """columns that stop at step 1, on a closing step, one step after it, later, and a zero right-hand side next to live columns: every
    frozen column keeps the x, history and count of its last step (the oracle column's), whatever check_every polls in between"""
    got = check_case(case)
    assert tuple(g[2] for g in got) == case.stops


@pytest.mark.parametrize("use_x0", [False, True])
@pytest.mark.parametrize("k", [6, 5])
def test_freezing_is_independent_of_check_every(k, use_x0):
    outs = [solve_multi(c, device_operator(c)) for c in CASES if c.group == "freeze" and len(c.rhs) == k and c.use_x0 == use_x0]
    assert len(outs) == 3
    for other in outs[1:]:
        for j in range(k):
            assert_same("column %d" % j, other[j], outs[0][j], nan=True)


# ---- c. use_x0 through every apply form -------------------------------------------------------------------------------------------
@by_group("x0")
def test_use_x0_through_every_apply_form(case):
    tag = case.id[3:].rsplit("-k", 1)[0]
    want = mc.X0_STORAGE[tag]
    A = device_operator(case)
    if want:
        lay = A.ell_layout()
        fmt, npat = A.storage_format()
        assert fmt == want["fmt"], (fmt, npat, lay)
        if "slots" in want:
            assert npat == want["slots"]
        if "lanes" in want:
            assert lay["lanes"] == want["lanes"]
        if "lanes_gt1" in want:
            assert lay["lanes"] > 1
        if "tail" in want:
            assert (lay["tail_rows"] > 0) == want["tail"]
        if "window" in want:       # (the single apply's LDS window; the k-wide apply has one slab kernel for both)
            assert lay["x_window"] == want["window"], lay
    got = check_case(case)
    if not case.bits:          # block-CSR: the oracle within the reordering sensitivity of its own sums
        Ao = mc.oracle_operator(case.spec, case.shift)
        po = orc.gcr_param(restart=case.restart, max_iter=case.max_iter, tol=case.tol, use_x0=True)
        for j in range(len(case.rhs)):
            ref, sens, _ = orc.gcr_reorder_sensitivity(Ao, po, mc.column(case.spec, case.rhs[j]), mc.column(case.spec, case.x0[j]))
            hist_close(got[j][1], ref, "%s column %d" % (case.id, j), sens)


# ---- d. plain-order territory -----------------------------------------------------------------------------------------------------
@by_group("plain")
def test_plain_order_territory(case):
    """where the single solve sums in another order (xr_fuse_kind 2: banded |r|^2 and start-up sums; the one-workgroup path at or below the
    small-solve limit) the batched solve sums |r|^2 and the start-up sums in the plain row order and the beta dots over the row map"""
    A = device_operator(case)
    n = mc.system(case.spec).N
    if case.spec[0] == "slab":
        assert A.xr_fuse_kind() == 2
        band, per = orc.row_map(n, A.ell_layout()["reach"])
        assert band == 256 * 256 and per == 64
    else:
        assert n <= SMALL_DEFAULT
    check_case(case)


def test_kind2_slab_is_the_smallest():
    nz = mc.KIND2_NZ - 1
    A = Sparse(*mg.problems.poisson3d_csr(256, ni=nz))
    assert A.xr_fuse_kind() != 2


# ---- e. reuse ---------------------------------------------------------------------------------------------------------------------
def test_work_storage_reused_from_solve_to_solve():
    """one GCR object, one process: the work storage survives (same n, k, slots: a shorter history inside the larger allocation) or is
    re-made (other k, other cycle length); nothing of an earlier solve may leak into a later one"""
    seq = mc.reuse_sequence()
    gcr = GCR(device_operator(seq[0]), GCR_Param(0, 5, 40, mc.FREEZE_TOL, False))
    outs = [check_case(c, gcr) for c in seq]
    assert tuple(g[2] for g in outs[0]) == seq[0].stops
    for j in range(len(seq[0].rhs)):
        assert_same("first against last, column %d" % j, outs[-1][j], outs[0][j])
