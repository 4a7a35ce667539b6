"""Even-odd hopping-parameter scans on the GPU: MultiEvenOddDiracOp (the Schur complements 1 - k_j^2 D_eo D_oe on column j of a
block; csrc/evenodd_multi.hip) through the k-wide apply, the block split / merge / prepare / reconstruct and the batched GCR.
Everything is compared bit for bit (np.array_equal) with the single entry points on an EvenOddDiracOp at ks[j] — the two rules
include/mgcr.h states for mgcr_eo_multi_create.  The single side walks ONE EvenOddDiracOp through the values with set_k, which
tests/test_gpu_evenodd.py shows to equal a fresh operator per value.  The shifts are distinct and partly complex (with equal shifts
a wrong column index would pass); the premises of the ladder are checked on the CPU in tests/test_evenodd_multi_cases.py."""
import ctypes as C

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, EvenOddDiracOp, Field, GCR, GCR_Param, MgcrError, MultiEvenOddDiracOp, MultiField, Sparse,
                                     _lib, stat)
from tests import evenodd_cases as ec
from tests import evenodd_multi_cases as emc

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 5, 8, 12, 16]           # masked K (5, 12), the tail's 8 + 4 windows (12), the widest block (16)
RULE1_CASES = ["sample", "open4d", "chain", "two_parts", "scalar", "scalar_ti", "grid2d_varied", "grid2d_const", "grid4d_const",
               "long", "tail", "lanes"]
RULE2_CASES = ["sample", "chain", "scalar", "grid2d_const", "long"]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_operators():
    yield
    _cache.clear()


def sparse(name):
    if ("D", name) not in _cache:
        c = emc.case(name)
        _cache[("D", name)] = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    return _cache[("D", name)]


def evenodd(name, role):
    """two EvenOddDiracOps per case: "multi", whose halves the block operators borrow, and "single", walked through the shifts"""
    key = ("eo", name, role)
    if key not in _cache:
        _cache[key] = EvenOddDiracOp(sparse(name), emc.case_k(name), emc.parity(name))
    return _cache[key]


def field(v):
    return Field((v.size,), v)


def block(cols):
    cols = np.asarray(cols)
    return MultiField((cols.shape[1],), cols.shape[0], cols)


def code_of(fn):
    with pytest.raises(MgcrError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- Rule 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RULE1_CASES)
def test_rule1_every_block_entry_point(name):
    c, m = emc.case(name), emc.case_plan(name)
    eo, single = evenodd(name, "multi"), evenodd(name, "single")
    n, ne, no = eo.sizes()
    assert (n, ne, no) == (c.n, m.even.size, m.odd.size)
    lay = [h.ell_layout() for h in eo.halves()]
    print("storage of %s: %s" % (name, [(h.storage_format(), l["lanes"], l["tail_rows"]) for h, l in zip(eo.halves(), lay)]))
    if name in ("long", "tail"):
        assert all(l["tail_rows"] > 0 for l in lay), lay
    if name == "long":
        assert all(emc.BIPARTITE["long"][1]["long_len"] > l["tail_chunk_cap"] + l["ell_width"] for l in lay), lay   # rows that fit no chunk
    if name == "lanes":
        assert all(l["lanes"] > 1 for l in lay), lay
    if name == "sample":
        assert lay[0]["lanes"] == 8, lay
    if name == "open4d":
        assert ne != no and ne % 64 != 0
    kmax = max(WIDTHS)
    ks = emc.shifts(name, kmax)
    xs = [ec.rhs(ne, 100 + j) for j in range(kmax)]           # a block of the even half
    bs = [ec.rhs(n, 200 + j) for j in range(kmax)]            # a full right-hand side
    os_ = [ec.rhs(no, 300 + j) for j in range(kmax)]          # a block of the odd half
    want = []                                                 # the single entry points, column by column (a column's shift does not depend on the width)
    for j in range(kmax):
        single.set_k(ks[j])
        x, b = field(xs[j]), field(bs[j])
        e, o = single.split(b)
        want.append(dict(apply=single(x).to_numpy(), prepare=single.prepare(b).to_numpy(), reconstruct=single.reconstruct(b, x).to_numpy(),
                         even=e.to_numpy(), odd=o.to_numpy(), merge=single.merge(x, field(os_[j])).to_numpy()))
    for k in WIDTHS:
        M = MultiEvenOddDiracOp(eo, ks[:k])
        assert M.ncols == k and M.get_dim() == M.get_nrow() == ne and _lib.lib().mgcr_op_nnz(M.h) == c.col.size
        X, B, O = block(xs[:k]), block(bs[:k]), block(os_[:k])
        E, Od = M.split(B)
        got = dict(apply=M.apply_multi(X).to_numpy(), prepare=M.prepare(B).to_numpy(), reconstruct=M.reconstruct(B, X).to_numpy(),
                   even=E.to_numpy(), odd=Od.to_numpy(), merge=M.merge(X, O).to_numpy())
        for what, arr in got.items():
            for j in range(k):
                assert np.array_equal(arr[j], want[j][what]), (what, k, j)
    # ... and the apply is the Schur complement of its column: the model agrees to rounding
    model = ec.schur_apply(m, ks[3], xs[3])
    assert np.abs(want[3]["apply"] - model).max() <= 1e-12 * np.abs(model).max()


# ---- Rule 2 -----------------------------------------------------------------------------------------------------------------------
TOL2 = 1e-8


@pytest.mark.parametrize("use_x0", [False, True], ids=["zero", "x0"])
@pytest.mark.parametrize("restart", [1, 5, 16])
@pytest.mark.parametrize("name", RULE2_CASES)
def test_rule2_batched_schur_solve(name, restart, use_x0):
    """mgcr_gcr_solve_multi on the operator, k = 5 and k = 12, against mgcr_gcr_solve on the single operator at ks[j].  max_iter is one
    more than the steps the quickest of the first five columns needs, found by solving those columns alone under a generous cap (on
    these operators the counts do not grow steadily with the shift): in either width that column stops early and others run into the cap —
    asserted on the single solves' counts."""
    m = emc.case_plan(name)
    eo, single = evenodd(name, "multi"), evenodd(name, "single")
    ne = m.even.size
    ks = emc.shifts(name, 12)
    bs = [ec.rhs(ne, 400 + j) for j in range(12)]
    x0 = [0.01 * ec.rhs(ne, 500 + j) if use_x0 else np.zeros(ne, ec.c128) for j in range(12)]
    free = []
    for j in range(5):
        single.set_k(ks[j])
        probe = GCR(single, GCR_Param(0, restart, 200, TOL2, False, use_x0=use_x0))
        probe.solve(field(bs[j]), field(x0[j]))
        free.append(probe.last_iterations)
    assert min(free) < 200, free
    prm = GCR_Param(0, restart, min(free) + 1, TOL2, False, use_x0=use_x0)
    ref = []
    for j in range(12):
        single.set_k(ks[j])
        x = field(x0[j])
        g = GCR(single, prm)
        g.solve(field(bs[j]), x)
        ref.append((g.last_history, g.last_iterations, g.last_converged, x.to_numpy()))
    its = [r[1] for r in ref]
    print("%s restart %d x0 %d: single iterations %s (uncapped %s), cap %d" % (name, restart, use_x0, its, free, prm.max_iter))
    assert min(its[:5]) < prm.max_iter and max(its[:5]) == prm.max_iter and max(its) == prm.max_iter, (free, its)
    for k in (5, 12):
        M = MultiEvenOddDiracOp(eo, ks[:k])
        X = block(x0[:k])
        g = GCR(M, prm)
        g.solve_multi(block(bs[:k]), X)
        Xh = X.to_numpy()
        for j in range(k):
            assert (g.last_iterations[j], g.last_converged[j]) == ref[j][1:3], (k, j, g.last_iterations, its)
            assert np.array_equal(g.last_history[j], ref[j][0]), (k, j)
            assert np.array_equal(Xh[j], ref[j][3]), (k, j)


# ---- the ladder -------------------------------------------------------------------------------------------------------------------
def ladder_param():
    return GCR_Param(0, emc.LADDER_RESTART, emc.LADDER_MAX_ITER, emc.LADDER_TOL, False)


def ladder_solve(M, bv, k):
    X = MultiField((bv.size,), k).set_zero()
    M.solve(block([bv] * k), X, ladder_param())
    return M.last_history, M.last_iterations, M.last_converged, X.to_numpy()


def test_the_ladder_on_the_sample():
    c, m = ec.case("sample"), ec.case_plan("sample")
    bv = ec.rhs(c.n)
    eo, single = evenodd("sample", "multi"), evenodd("sample", "single")
    k = len(emc.LADDER)
    hist, its, conv, Xh = ladder_solve(MultiEvenOddDiracOp(eo, emc.LADDER), bv, k)
    print("ladder iterations %s (model %s)" % (its, emc.LADDER_MODEL_STOPS))
    for j, kj in enumerate(emc.LADDER):
        single.set_k(kj)
        x = Field((c.n,)).set_zero()
        single.solve(field(bv), x, ladder_param())
        assert (its[j], conv[j]) == (single.last_iterations, single.last_converged), (j, its)
        assert np.array_equal(hist[j], single.last_history), j
        assert np.array_equal(Xh[j], x.to_numpy()), j
    assert len(set(its)) == k and its.count(emc.LADDER_MAX_ITER) == 1, its
    assert conv == [i != emc.LADDER_MAX_ITER for i in its]
    for j, kj in enumerate(emc.LADDER):            # the bounds of tests/test_gpu_evenodd.py::test_solve_against_the_full_system
        if not conv[j]:
            continue
        xfull = Field((c.n,)).set_zero()
        g = GCR(DiracOp(sparse("sample"), kj), GCR_Param(0, 5, 4000, emc.LADDER_TOL, False))
        g.solve(field(bv), xfull)
        err = np.linalg.norm(Xh[j] - xfull.to_numpy()) / np.linalg.norm(xfull.to_numpy())
        r = ec.dirac_apply(c, kj, Xh[j]) - bv
        odd = np.linalg.norm(r[m.odd]) / np.linalg.norm(bv)
        print("k = %r: %d steps, |x - x_full| / |x_full| = %.3e, odd-half residual %.3e" % (kj, its[j], err, odd))
        assert g.last_converged and err <= 10 * emc.LADDER_TOL, (kj, err)
        assert odd <= 1e-13, (kj, odd)


# ---- set_k ------------------------------------------------------------------------------------------------------------------------
def test_set_k_equals_a_fresh_operator_and_leaves_enqueued_work_alone():
    c, m = ec.case("sample"), ec.case_plan("sample")
    eo = evenodd("sample", "multi")
    old, new = [0.05, 0.08 + 0.02j, 0.11], [0.12 - 0.03j, 0.06, 0.09 + 0.01j]
    bv = ec.rhs(c.n)
    X = block([ec.rhs(m.even.size, 600 + j) for j in range(3)])
    M = MultiEvenOddDiracOp(eo, old)
    y_old = MultiEvenOddDiracOp(eo, old).apply_multi(X).to_numpy()
    y_new = MultiEvenOddDiracOp(eo, new).apply_multi(X).to_numpy()
    assert not np.array_equal(y_old, y_new)
    Y = M.apply_multi(X)               # enqueued, not waited for: its launches carry the old values
    M.set_k(new)
    assert np.array_equal(Y.to_numpy(), y_old)
    assert np.array_equal(M.apply_multi(X).to_numpy(), y_new)
    after, fresh = ladder_solve(M, bv, 3), ladder_solve(MultiEvenOddDiracOp(eo, new), bv, 3)
    before = ladder_solve(MultiEvenOddDiracOp(eo, old), bv, 3)
    assert after[1:3] == fresh[1:3] and np.array_equal(after[3], fresh[3])
    assert all(np.array_equal(a, f) for a, f in zip(after[0], fresh[0]))
    assert not np.array_equal(after[3], before[3])
    assert code_of(lambda: M.set_k([0.1, 0.2]))[0] == 1


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors():
    lib = _lib.lib()
    c, m = ec.case("open4d"), ec.case_plan("open4d")        # n_e != n_o: an odd-sized block is a wrong length for the even half
    eo = evenodd("open4d", "multi")
    n, ne, no = c.n, m.even.size, m.odd.size
    ks = emc.shifts("open4d", 3)
    M = MultiEvenOddDiracOp(eo, ks)
    Z = lambda rows, k=3: MultiField((rows,), k).set_zero()             # noqa: E731
    p = GCR_Param(0, 5, 5, 1e-10, False)
    # creation
    for bad in ([], [0.1] * 17, [0.1, 0.0, 0.2]):
        assert code_of(lambda: MultiEvenOddDiracOp(eo, bad))[0] == 1, bad
    code, msg = code_of(lambda: M.set_k([0.1, 0.0, 0.2]))
    assert code == 1 and "No k value" in msg
    assert code_of(lambda: MultiEvenOddDiracOp(sparse("open4d"), ks))[0] == 1                  # not an EvenOddDiracOp
    assert code_of(lambda: MultiEvenOddDiracOp(DiracOp(sparse("open4d"), 0.1), ks))[0] == 1
    # the column count against nk
    wrong_width = [lambda: M.apply_multi(Z(ne, 2), Z(ne, 2)), lambda: GCR(M, p).solve_multi(Z(ne, 2), Z(ne, 2)),
                   lambda: M.bench_apply_multi(Z(ne, 2), Z(ne, 2), 1), lambda: M.split(Z(n, 2)), lambda: M.split(Z(n), Z(ne, 2), Z(no)),
                   lambda: M.merge(Z(ne), Z(no, 4)), lambda: M.prepare(Z(n, 2)), lambda: M.reconstruct(Z(n), Z(ne, 2)),
                   lambda: M.solve(Z(n, 2), Z(n, 2), p), lambda: M.solve(Z(n), Z(n, 4), p)]
    # the block lengths
    wrong_rows = [lambda: M.apply_multi(Z(no), Z(no)), lambda: M.apply_multi(Z(ne), Z(no)), lambda: GCR(M, p).solve_multi(Z(no), Z(no)),
                  lambda: GCR(M, p).solve_multi(Z(ne), Z(n)), lambda: M.split(Z(n - 1)), lambda: M.split(Z(n), Z(no), Z(no)),
                  lambda: M.split(Z(n), Z(ne), Z(ne)), lambda: M.merge(Z(no), Z(no)), lambda: M.merge(Z(ne), Z(no), Z(n + 1)),
                  lambda: M.prepare(Z(ne)), lambda: M.prepare(Z(n), Z(no)), lambda: M.reconstruct(Z(ne), Z(ne)),
                  lambda: M.reconstruct(Z(n), Z(no)), lambda: M.reconstruct(Z(n), Z(ne), Z(ne)), lambda: M.solve(Z(ne), Z(n), p),
                  lambda: M.solve(Z(n), Z(ne), p)]
    # aliasing
    A, F = Z(ne), Z(n)
    aliased = [lambda: M.apply_multi(A, A), lambda: GCR(M, p).solve_multi(A, A), lambda: M.solve(F, F, p), lambda: M.prepare(F, F),
               lambda: M.reconstruct(F, A, F)]
    for i, call in enumerate(wrong_width + wrong_rows + aliased):
        assert code_of(call)[0] == 1, i
    # the entry points that work on one Field, the queue, multigrid and the layout queries: MGCR_ERR_UNSUPPORTED, naming the kind
    f, y = Field((ne,)).set_zero(), Field((ne,)).set_zero()
    refused = [lambda: M(f, out=y), lambda: M.bench_apply(f, y, 1), lambda: GCR(M, p).solve(f, y), lambda: GCR(M, p)(f, out=y),
               lambda: GCR(M, p).solve_queue([f], [y], width=1), M.storage_format, M.ell_layout, M.stored_bytes, M.xr_fuse_kind]
    for i, call in enumerate(refused):
        code, msg = code_of(call)
        assert code == 7 and "MultiEvenOddDiracOp" in msg, (i, code, msg)
    pc = p._c()
    h = C.c_void_p()
    assert lib.mgcr_gcr_create(M.h, C.byref(pc), 1, C.byref(h)) == 7 and not h.value
    assert b"MultiEvenOddDiracOp" in lib.mgcr_last_error()
    assert lib.mgcr_gcr_solve(M.h, C.byref(pc), f.h, y.h, None, 0, None, None) == 7
    g = GCR(sparse("open4d"), p)
    assert lib.mgcr_gcr_set_operator(g.h, M.h) == 7
    assert lib.mgcr_mg_create(M.h, C.byref(_lib.MgParamC()), C.byref(h)) == 7 and not h.value
    assert b"MultiEvenOddDiracOp" in lib.mgcr_last_error()
    # the restrictions of the batched solve
    assert code_of(lambda: M.solve(Z(n), Z(n), GCR_Param(4, 0, 5, 1e-10, False)))[0] == 7      # truncation mode
    assert code_of(lambda: M.solve(Z(n), Z(n), GCR_Param(0, 20, 50, 1e-10, False)))[0] == 7     # a cycle longer than 16
    # the plain EvenOddDiracOp goes on refusing blocks
    assert code_of(lambda: eo.apply_multi(Z(ne), Z(ne)))[0] == 7
    assert code_of(lambda: GCR(eo, p).solve_multi(Z(ne), Z(ne)))[0] == 7


# ---- counters ---------------------------------------------------------------------------------------------------------------------
def test_counters():
    c = ec.case("chain")                                    # 23 even rows: small enough for the one-workgroup solve of a Sparse
    eo = evenodd("chain", "multi")
    ks = emc.shifts("chain", 4)
    M = MultiEvenOddDiracOp(eo, ks)
    still = ("small_solves", "resident_solves", "step_build_launches")
    before = {k: stat(k) for k in still + ("multi_solves",)}
    X = MultiField((c.n,), 4).set_zero()
    M.solve(block([ec.rhs(c.n, 700 + j) for j in range(4)]), X, GCR_Param(0, 5, 200, 1e-10, False))
    assert all(M.last_converged), M.last_iterations
    assert stat("multi_solves") == before["multi_solves"] + 1
    assert {k: stat(k) for k in still} == {k: before[k] for k in still}
