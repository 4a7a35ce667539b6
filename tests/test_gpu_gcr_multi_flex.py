"""The flexible batched GCR on the GPU: mgcr_gcr_solve_multi with a flexible right preconditioner (csrc/gcr_multi.hip, the device
side csrc/gcr_multi_flex.hip).

Rule F — history, iteration count, convergence flag and x of column j of GCR(A, GCR_Param(..., solver_r=M, flexible=True))
.solve_multi have the BITS of .solve on column j alone with the same M in the slot:
  slot kind (a), a LowPrecisionGCR: cases f (45 rows, less than a wave), b (315 rows, odd n, real slab), d (1152 rows, complex
  slab), e (3001 rows, tail rows), a (the 3072-row sample at 0.15 and 0.18); the inner settings INNER and, on case a,
  INNER_TWO_RESTARTS; widths 1, 3, 5, 16 of the 16-column block of tests/gcr_multi_flex_cases.py (a zero column, a duplicate, columns
  that stop at different outer steps through use_x0); use_x0 on and off; the premise blocks — restart 5 (a column frozen inside a
  cycle with x updates pending while others run a cycle more: what an exit kernel without the mask corrupts), restart 3 (columns
  that stop on a closing step), restart 1, max_iter < restart, max_iter reached;
  slot kind (b): a Sparse and a DiracOp as M (the masked copy);
  a MultiDiracOp as A against DiracOp(D, k_j) singles.
Work storage reused by a second solve and by an unpreconditioned solve after a flexible one: bits unchanged.  The gate: behind a solve
in which every column converges last_multi reports 0 steps for every column; in the max_iter block the converged columns report 0
and the running ones more.  The counters.  Every refusal with its code, x untouched.  No tolerance appears: everything compared is
bits — but for the zero column, whose history and x are NaN (0 / 0) on both sides: NaN against NaN, position by position."""
import ctypes as C

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, Field, GCR, GCR_Param, LowPrecisionEvenOddGCR, LowPrecisionGCR, MgcrError, MultiDiracOp,
                                     MultiEvenOddDiracOp, EvenOddDiracOp, MultiField, Sparse, _lib, stat)
from tests import gcr32_cases as g
from tests import gcr_multi_flex_cases as fc

pytestmark = pytest.mark.gpu

_cache = {}
F_CASES = (("f", 0.45), ("b", None), ("d", 0.09), ("e", 0.18), ("a", 0.15), ("a", 0.18))
F_KEYS = [(name, k, inner) for name, k in F_CASES for inner in g.inner_settings(name)]


@pytest.fixture(scope="module", autouse=True)
def release():
    yield
    _cache.clear()


def sparse(name):
    if ("M", name) not in _cache:
        n, rp, ci, va = g.matrix(name)
        _cache[("M", name)] = Sparse(n, n, rp, ci, va)
    return _cache[("M", name)]


def low(name, k, inner=g.INNER[0]):
    return LowPrecisionGCR(sparse(name), k, GCR_Param(0, inner[0], inner[1], inner[2], False))


def operator(name, k):
    return sparse(name) if k is None else DiracOp(sparse(name), k)


def field(v):
    return Field((v.size,), v)


def block(cols):
    cols = np.ascontiguousarray(cols, np.complex128)
    return MultiField((cols.shape[1],), cols.shape[0], cols)


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


def code_of(fn):
    with pytest.raises(MgcrError) as e:
        fn()
    return e.value.code, str(e.value)


def param(outer, M=None, use_x0=False, **kw):
    restart, max_it, tol = outer
    return GCR_Param(0, restart, max_it, tol, False, solver_r=M, flexible=M is not None, use_x0=use_x0, **kw)


def single(A, M, outer, b, x0, use_x0):
    """(x, history, iterations, converged) of the single solve on one column"""
    s = GCR(A, param(outer, M, use_x0))
    x = field(x0)
    s.solve(field(b), x)
    return x.to_numpy().reshape(-1), s.last_history, s.last_iterations, s.last_converged


def batched(A, M, outer, B, X0, use_x0):
    s = GCR(A, param(outer, M, use_x0))
    X = block(X0)
    s.solve_multi(block(B), X)
    return X.to_numpy(), s.last_history, s.last_iterations, s.last_converged


def assert_rule_f(got, refs, what, B):
    xs, hist, its, conv = got
    for j, (x, h, it, cv) in enumerate(refs):
        assert its[j] == it and conv[j] == cv, (what, j, its[j], it, conv[j], cv)
        if not B[j].any():
            # the zero column: 0 / 0 — history and x are NaN in the single solve and in this column alike, and a NaN has no value: which
            # sign bit it carries depends on the operand order the compiler chose in each kernel (tests/test_gpu_multi_rhs_edges.py
            # compares the unpreconditioned solve's zero column the same way)
            assert np.array_equal(np.asarray(hist[j]), np.asarray(h), equal_nan=True), (what, j, hist[j], h)
            assert np.array_equal(xs[j], x, equal_nan=True), (what, j)
            continue
        assert np.array_equal(np.asarray(hist[j]).view(np.uint64), np.asarray(h).view(np.uint64)), (what, j, hist[j], h)
        assert np.array_equal(bits(xs[j]), bits(x)), (what, j)


def check_widths(A, M, outer, blk, widths, use_x0s=(True, False), what=""):
    """Rule F at every width, the singles computed once per column; returns the singles' iteration counts (use_x0 on)"""
    counts = None
    for use_x0 in use_x0s:
        refs = [single(A, M, outer, blk.B[j], blk.X0[j], use_x0) for j in range(max(widths))]
        for w in widths:
            assert_rule_f(batched(A, M, outer, blk.B[:w], blk.X0[:w], use_x0), refs[:w], (what, "width", w, "use_x0", use_x0), blk.B)
        if counts is None:
            counts = [r[2] for r in refs]
    return counts


# ---- Rule F, slot kind (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", F_KEYS, ids=lambda key: "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1]))
def test_rule_f_every_column_has_the_single_solves_bits(key):
    name, k, inner = key
    blk = fc.make_block(name, k, fc.COLUMNS)
    counts = check_widths(operator(name, k), low(name, k, inner), fc.OUTER_5, blk, fc.WIDTHS, what=key)
    print(key, "outer steps per column", counts)
    assert counts[2] == 1 and counts[3] == counts[0]                      # the zero column ends at its first test; the duplicate


PREMISE_OUTERS = {"restart5": fc.OUTER_5, "restart3": fc.OUTER_3, "restart1": fc.OUTER_1, "short": fc.OUTER_SHORT, "limit": fc.OUTER_LIMIT}


@pytest.mark.parametrize("which", list(PREMISE_OUTERS))
def test_rule_f_the_premise_blocks(which):
    """the blocks whose premises tests/test_gcr_multi_flex_cases.py checks on the model — and here on the device's own counts"""
    name, k, inner = fc.PREMISE
    outer = PREMISE_OUTERS[which]
    restart, max_iter, _ = outer
    blk = fc.make_block(name, k, fc.COLUMNS)
    its = check_widths(operator(name, k), low(name, k, inner), outer, blk, (5, 16), use_x0s=(True,), what=which)
    print(which, "outer steps per column", its)
    if which in ("restart5", "restart3"):
        assert fc.pending_and_runner(its[:5], restart, max_iter), its    # (i): frozen inside a cycle, others a cycle more
    if which == "restart3":
        assert any(s % restart == 0 and s < max(its) for s in its[:5]), its    # (ii): frozen on a closing step
    if which == "short":
        assert max(its) == max_iter < restart
    if which == "limit":
        assert its[0] == max_iter and any(1 < s < max_iter for s in its[:5]), its


# ---- slot kind (b), a MultiDiracOp as A --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("a", 0.15), ("d", 0.09), ("b", None)])
def test_rule_f_a_sparse_in_the_slot(name, k):
    """M = the stored matrix D itself: a poor preconditioner and a linear map.  The "mid" columns stop at once and stay frozen, one x
    update pending, while the others run into max_iter: the masked copy"""
    blk = fc.make_block(name, k, fc.COLUMNS)
    its = check_widths(operator(name, k), sparse(name), (5, 30, 1e-10), blk, fc.WIDTHS, what=(name, "Sparse"))
    print(name, "Sparse in the slot: outer steps per column", its)
    assert max(its) - min(s for s in its if s % 5) >= 5


@pytest.mark.parametrize("name,k", [("a", 0.15), ("e", 0.18)])
def test_rule_f_a_dirac_op_in_the_slot(name, k):
    """M = 1 + k D, the first two terms of the inverse's series: columns stop all over the cycles"""
    blk = fc.make_block(name, k, fc.COLUMNS)
    its = check_widths(operator(name, k), DiracOp(sparse(name), -k), fc.OUTER_5, blk, (5, 16), what=(name, "DiracOp"))
    print(name, "DiracOp in the slot: outer steps per column", its)
    assert fc.pending_and_runner(its, 5, fc.OUTER_5[1]), its


@pytest.mark.parametrize("slot", ["low", "sparse"])
def test_rule_f_a_multi_dirac_op_against_dirac_op_singles(slot):
    name, inner = "a", g.INNER[0]
    ks = [0.15, 0.18, 0.10, 0.15, 0.12 + 0.02j]
    blk = fc.make_block(name, 0.15, fc.COLUMNS[:5])
    M = low(name, 0.15, inner) if slot == "low" else sparse(name)          # one k32 for all columns: a preconditioner at another k
    outer = fc.OUTER_5 if slot == "low" else (5, 30, 1e-10)
    for use_x0 in (True, False):
        refs = [single(DiracOp(sparse(name), ks[j]), M, outer, blk.B[j], blk.X0[j], use_x0) for j in range(5)]
        for w in (3, 5):
            got = batched(MultiDiracOp(sparse(name), ks[:w]), M, outer, blk.B[:w], blk.X0[:w], use_x0)
            assert_rule_f(got, refs[:w], (slot, w, use_x0), blk.B)
    print(slot, "MultiDiracOp: outer steps per column", [r[2] for r in refs])


# ---- work storage, gate, counters ----------------------------------------------------------------------------------------------------
def test_reused_work_storage_and_an_unpreconditioned_solve_after_a_flexible_one():
    name, k, inner = fc.PREMISE
    A, M = operator(name, k), low(name, k, inner)
    blk = fc.make_block(name, k, fc.COLUMNS[:5])
    plain0 = batched(A, None, (5, 20, 1e-10), blk.B, blk.X0, True)         # (storage made without the block z)
    first = batched(A, M, fc.OUTER_5, blk.B, blk.X0, True)
    second = batched(A, M, fc.OUTER_5, blk.B, blk.X0, True)
    plain1 = batched(A, None, (5, 20, 1e-10), blk.B, blk.X0, True)         # (on the flexible solve's storage)
    third = batched(A, M, fc.OUTER_5, blk.B, blk.X0, True)
    for a, b in ((first, second), (first, third), (plain0, plain1)):
        assert a[2] == b[2] and a[3] == b[3]
        assert np.array_equal(bits(a[0]), bits(b[0]))
        assert all(np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64)) for p, q in zip(a[1], b[1]))
    # ... and the unpreconditioned solve still has the single solve's bits
    refs = [single(A, None, (5, 20, 1e-10), blk.B[j], blk.X0[j], True) for j in range(5)]
    assert_rule_f(plain1, refs, "unpreconditioned after flexible", blk.B)


def test_the_gate_cuts_the_inner_solves_nobody_reads():
    name, k, inner = fc.PREMISE
    A, M = operator(name, k), low(name, k, inner)
    blk = fc.make_block(name, k, fc.COLUMNS[:5])
    names = ("multi_flex_solves", "multi_solves", "gcr32_multi_applies", "gcr32_multi_steps", "gcr32_applies")
    before = [stat(s) for s in names]
    _, _, its, conv = batched(A, M, fc.OUTER_5, blk.B, blk.X0, True)
    after = [stat(s) for s in names]
    assert all(conv)
    # the apply behind the last update was cut for every column: frozen, or about to end on that residual
    assert [l[0] for l in M.last_multi()] == [0] * 5, M.last_multi()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1 and after[4] == before[4]
    applies = after[2] - before[2]
    assert applies >= max(its) and after[3] - before[3] == applies * inner[1]     # the start's apply + one per step but the last
    # the max_iter block: the converged columns report 0 steps, the running ones more
    _, _, its, conv = batched(A, M, fc.OUTER_LIMIT, blk.B, blk.X0, True)
    last = [l[0] for l in M.last_multi()]
    print("limit block: outer steps", its, "converged", conv, "inner steps of the last apply", last)
    assert not all(conv) and any(conv)
    for j in range(5):
        assert (last[j] == 0) == conv[j], (j, last, conv)
    # an unpreconditioned solve moves none of the flexible counters
    mid = [stat(s) for s in names]
    batched(A, None, (5, 20, 1e-10), blk.B, blk.X0, True)
    end = [stat(s) for s in names]
    assert end[0] == mid[0] and end[1] == mid[1] + 1 and end[2:] == mid[2:]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_its_code_and_x_untouched():
    name, k = "f", 0.45
    c = g.case(name, k)
    A, M = operator(name, k), low(name, k)
    blk = fc.make_block(name, k, fc.COLUMNS[:3])
    B, X = block(blk.B), block(blk.B[::-1])
    ref = X.to_numpy()
    L = _lib.lib()

    def code(p, A_=A, B_=B, X_=X):
        pc = p._c()
        return L.mgcr_gcr_solve_multi(A_.h, C.byref(pc), B_.h, X_.h, None, 0, None, None)

    inner_gcr = GCR(A, GCR_Param(0, 5, 2, 1e-8, False))
    eo_low = LowPrecisionEvenOddGCR(sparse(name), k, GCR_Param(0, 8, 8, 0.1, False))
    other = low("b", None)                                                    # 315 rows
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_l=M)) == 7            # a left preconditioner
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_l=sparse(name))) == 7
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=M)) == 7            # a right preconditioner with flexible == 0
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=sparse(name))) == 7
    assert code(GCR_Param(0, 5, 10, 1e-8, False, flexible=True)) == 7         # flexible without one, as before
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=inner_gcr, flexible=True)) == 7      # a GCR object in either slot
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_l=inner_gcr)) == 7
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=eo_low, flexible=True)) == 7         # an even-odd low
    assert code(GCR_Param(0, 5, 10, 1e-8, False), A_=M) == 7                                   # a low-precision GCR as A
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=M, flexible=True), A_=M) == 7
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=M, flexible=True, profile_spmv=True)) == 7
    assert code(GCR_Param(4, 0, 10, 1e-8, False, solver_r=M, flexible=True)) == 7              # truncation mode
    assert code(GCR_Param(0, 0, 10, 1e-8, False, solver_r=M, flexible=True)) == 7              # full mode
    assert code(GCR_Param(0, 17, 40, 1e-8, False, solver_r=M, flexible=True)) == 7             # a cycle longer than 16
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=MultiDiracOp(sparse(name), [0.1, 0.2, 0.3]), flexible=True)) == 7
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=other, flexible=True)) == 1          # a dimension that is not n
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=sparse("b"), flexible=True)) == 1
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=M, flexible=True), X_=MultiField((c.n,), 2)) == 1
    cd, msg = code_of(lambda: GCR(A, GCR_Param(0, 5, 10, 1e-8, False, solver_r=other, flexible=True)).solve_multi(B, X))
    assert cd == 1 and "rows" in msg
    assert np.array_equal(bits(X.to_numpy()), bits(ref))                      # X untouched by all of these
    # the other batched and queued solves go on refusing every preconditioner
    pc = GCR_Param(0, 5, 10, 1e-8, False, solver_r=M, flexible=True)._c()
    b, x = field(blk.B[0]), Field((c.n,)).set_zero()
    hs, xs = (C.c_void_p * 1)(b.h), (C.c_void_p * 1)(x.h)
    kk = (C.c_double * 2)(k, 0.)
    assert L.mgcr_gcr_solve_queue(A.h, C.byref(pc), 1, 1, hs, xs, None, None, 0, None, None) == 7
    eo = EvenOddDiracOp(sparse(name), k)
    assert L.mgcr_eo_solve_queue(eo.h, C.byref(pc), 1, 1, hs, xs, kk, None, 0, None, None) == 7
    Mk = MultiEvenOddDiracOp(eo, [k, 0.5 * k])
    XF, YF = MultiField((c.n,), 2), MultiField((c.n,), 2)
    assert L.mgcr_eo_multi_solve(Mk.h, C.byref(pc), XF.h, YF.h, None, 0, None, None) == 7
    assert not x.to_numpy().any()
    # ... and the accepted call works afterwards
    assert code(GCR_Param(0, 5, 10, 1e-8, False, solver_r=M, flexible=True)) == 0
