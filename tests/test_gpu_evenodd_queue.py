"""The queued even-odd scan on the GPU (mgcr_eo_solve_queue, csrc/evenodd_queue.hip): any number of systems (1 - k_s D) x_s = b_s on
full Fields through `width` columns of ONE batched solve of the Schur systems.  Every comparison is bit for bit (np.array_equal)
with EvenOddDiracOp(D, k_s).solve on the system alone — history, iteration count, convergence flag and the WHOLE x — the rule
include/mgcr.h states.  The queue runs on one EvenOddDiracOp per case ("multi"), the single solves on a second one ("single") that
is walked through the values with set_k; they are computed once per module, shared and never changed.

The ladders are those of tests/evenodd_queue_cases.py.  At every width strictly between 1 and the number of systems the premise is
asserted on the single solves' own iteration counts: a system is admitted after step 0 beside a running column, and a column
retires at a cycle boundary at which another goes on (tests/test_evenodd_queue_cases.py checks it on the numpy model)."""
import ctypes as C

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, EvenOddDiracOp, Field, GCR, GCR_Param, MgcrError, MultiEvenOddDiracOp, MultiField, Sparse,
                                     _lib, experiments, read_data, stat)
from tests import evenodd_cases as ec
from tests import evenodd_multi_cases as emc
from tests import evenodd_queue_cases as eq
from tests import queue_cases as qc

pytestmark = pytest.mark.gpu

_cache = {}
_singles = {}


@pytest.fixture(scope="module", autouse=True)
def release_operators():
    yield
    _cache.clear()
    _singles.clear()


def sparse(name):
    if ("D", name) not in _cache:
        c = emc.case(name)
        _cache[("D", name)] = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    return _cache[("D", name)]


def evenodd(name, role):
    """two EvenOddDiracOps per case: "multi", whose halves the queue borrows, and "single", walked through the hopping parameters"""
    key = ("eo", name, role)
    if key not in _cache:
        _cache[key] = EvenOddDiracOp(sparse(name), emc.case_k(name), emc.parity(name))
    return _cache[key]


def param(restart, max_iter, tol, use_x0=False, check_every=0):
    return GCR_Param(0, restart, max_iter, tol, False, use_x0=use_x0, check_every=check_every)


def single(case, k, b, restart, max_iter, tol, x0=None, use_x0=False, tag=""):
    """(iterations, converged, history, x_full) of mgcr_eo_solve on the system alone; computed once per key and never changed"""
    key = (case, complex(k), restart, max_iter, tol, use_x0, tag)
    if key not in _singles:
        eo = evenodd(case, "single")
        eo.set_k(k)
        x = Field((b.size,), x0) if x0 is not None else Field((b.size,)).set_zero()
        eo.solve(Field((b.size,), b), x, param(restart, max_iter, tol, use_x0))
        res = (eo.last_iterations, eo.last_converged, eo.last_history.copy(), x.to_numpy())
        for a in res[2:]:
            a.setflags(write=False)
        _singles[key] = res
    return _singles[key]


def run_queue(case, ks, bs, refs, width, prm, x0s=None):
    """runs the queue on the "multi" operator and compares every system with its single solve; returns (steps, admissions) of the call"""
    eo = evenodd(case, "multi")
    n = eo.sizes()[0]
    fields = {}
    rhs = [fields.setdefault(id(b), Field((n,), b)) for b in bs]       # one Field per distinct right-hand side: handles repeat
    xs = [Field((n,), x0s[s]) if x0s is not None else Field((n,)).set_zero() for s in range(len(bs))]
    names = ("eo_queue_steps", "eo_queue_admissions", "eo_queue_solves", "queue_solves", "queue_steps", "queue_admissions", "multi_solves")
    before = [stat(c) for c in names]
    eo.solve_queue(rhs, xs, ks, prm, width=width)
    after = [stat(c) for c in names]
    assert after[2] == before[2] + 1 and after[3:] == before[3:]
    for s, (it, conv, hist, x) in enumerate(refs):
        assert eo.last_iterations[s] == it, (s, eo.last_iterations, [r[0] for r in refs])
        assert eo.last_converged[s] == conv, s
        assert np.array_equal(eo.last_history[s], hist), s
        assert np.array_equal(xs[s].to_numpy(), x), s
    return after[0] - before[0], after[1] - before[1]


def ladder_refs(name, use_x0=False, with_x0=False, tag=""):
    lad = eq.LADDERS[name]
    bs_by_seed = {}
    bs, x0s, refs = [], [], []
    for s, k in enumerate(lad.ks):
        b = eq.rhs_of(name, s)
        b = bs_by_seed.setdefault(b.tobytes(), b)                      # a shared right-hand side is ONE array (one Field)
        bs.append(b)
        x0s.append(eq.x0_of(name, s) if with_x0 else None)
        refs.append(single(lad.case, k, b, lad.restart, lad.max_iter, lad.tol, x0s[-1], use_x0, tag))
    return lad, bs, (x0s if with_x0 else None), refs


def check_ladder(name, use_x0=False, with_x0=False, tag="", check_every=0, widths=None):
    lad, bs, x0s, refs = ladder_refs(name, use_x0, with_x0, tag)
    its = [r[0] for r in refs]
    print("%s: single iterations %s" % (name, its))
    interior = eq.interior_widths(lad)
    assert interior, name
    for w in interior:
        assert eq.premise(its, w, lad.restart) == (True, True), (name, w, its)
    for w in (widths or lad.widths):
        steps, admissions = run_queue(lad.case, lad.ks, bs, refs, w, param(lad.restart, lad.max_iter, lad.tol, use_x0, check_every), x0s)
        assert admissions == len(its) - min(w, len(its)), (name, w, admissions)
    return its, refs


# ---- 1: the sample ladder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample", "sample_longest_first", "sample_shuffled"])
def test_the_sample_ladder(name):
    """widths 1, 2, 3, 6 and 16 (> nsys); one right-hand side shared by all systems; one column ends at the cap"""
    its, refs = check_ladder(name)
    assert its.count(emc.LADDER_MAX_ITER) == 1 and len(set(its)) == len(its), its
    assert [r[1] for r in refs] == [it != emc.LADDER_MAX_ITER for it in its]


# ---- 2: more systems than 16 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scalar20", "chain20"])
def test_more_systems_than_columns_of_a_block(name):
    lad = eq.LADDERS[name]
    assert len(lad.ks) == 20 and any(complex(k).imag != 0 for k in lad.ks)
    if name == "scalar20":
        assert all(h.ell_layout()["lanes"] == 1 for h in evenodd("scalar", "multi").halves())       # one thread per row: the fused stage 2
        before = stat("evenodd_fused_steps")
    its, refs = check_ladder(name)
    if name == "scalar20":
        assert stat("evenodd_fused_steps") > before                    # ... which the single solves took
    assert all(r[1] for r in refs)


# ---- 3: x on entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_x0", [True, False], ids=["use_x0", "ignored"])
@pytest.mark.parametrize("name", ["sample_x0", "open4d_x0"])
def test_nonzero_x_on_entry(name, use_x0):
    if name == "open4d_x0":
        _, ne, no = evenodd("open4d", "multi").sizes()
        assert ne != no
    check_ladder(name, use_x0=use_x0, with_x0=True, tag="x0")


# ---- 4: the storage forms of the halves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["long", "lanes", "grid2d_const", "scalar_ti", "two_parts"])
def test_storage_forms(name):
    eo = evenodd(name, "multi")
    lay = [h.ell_layout() for h in eo.halves()]
    fmt = [h.storage_format() for h in eo.halves()]
    print("storage of %s: %s" % (name, [(f, l["lanes"], l["tail_rows"]) for f, l in zip(fmt, lay)]))
    if name == "long":
        assert all(l["tail_rows"] > 0 for l in lay), lay              # the sub-scaled route at admission and at retirement
    if name == "lanes":
        assert all(l["lanes"] > 1 for l in lay), lay
    assert len(eq.LADDERS[name].ks) >= 5
    check_ladder(name)


# ---- 5: check_every --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_every", [0, 1, 7])
def test_check_every_does_not_change_the_results(check_every):
    check_ladder("sample_longest_first", check_every=check_every, widths=(2,))


# ---- 6: a column's own last step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [20, 23, 3])       # the last step closes a cycle / falls in mid-cycle / the cycle never closes
def test_every_system_runs_to_the_cap(max_iter):
    ks = emc.LADDER[:5]
    b = ec.rhs(ec.case("sample").n)
    refs = [single("sample", k, b, 5, max_iter, 0.0) for k in ks]
    assert [r[0] for r in refs] == [max_iter] * 5 and not any(r[1] for r in refs)
    steps, admissions = run_queue("sample", ks, [b] * 5, refs, 2, param(5, max_iter, 0.0))
    assert admissions == 3
    if max_iter == 3:
        assert steps == 9                               # three groups, each admitted at once when the one before has ended


# ---- 7: the shortest and the longest cycle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [1, 16])
def test_restart_1_and_16(restart):
    ks = eq.spread("scalar", 7, 3)
    n = ec.case("scalar").n
    bs = [ec.rhs(n, 900 + s) for s in range(7)]
    refs = [single("scalar", k, bs[s], restart, 200, 1e-10) for s, k in enumerate(ks)]
    its = [r[0] for r in refs]
    print("restart %d: single iterations %s" % (restart, its))
    assert len(set(its)) >= 3 and max(its) < 200, its
    run_queue("scalar", ks, bs, refs, 3, param(restart, 200, 1e-10))


# ---- 8: the work storage is kept and shared ------------------------------------------------------------------------------------------------
def test_reuse_with_other_batched_solves_in_between():
    lad, bs, _, refs = ladder_refs("sample")
    prm = param(lad.restart, lad.max_iter, lad.tol)
    run_queue("sample", lad.ks, bs, refs, 2, prm)
    # the batched even-odd solve at the same n_e, width and cycle length: the same storage
    eo = evenodd("sample", "multi")
    n = eo.sizes()[0]
    M = MultiEvenOddDiracOp(eo, lad.ks[:2])
    X = MultiField((n,), 2).set_zero()
    M.solve(MultiField((n,), 2, np.array([bs[0], bs[1]])), X, prm)
    for j in range(2):
        assert M.last_iterations[j] == refs[j][0] and np.array_equal(M.last_history[j], refs[j][2]) and np.array_equal(X.to_numpy()[j], refs[j][3])
    # ... and the queue of full-system solves on the Sparse, against the single solves with DiracOp(D, k)
    D = sparse("sample")
    short = lad.ks[:3]
    full_refs = []
    for k in short:
        x = Field((n,)).set_zero()
        g = GCR(DiracOp(D, k), prm)
        g.solve(Field((n,), bs[0]), x)
        full_refs.append((g.last_iterations, g.last_history.copy(), x.to_numpy()))
    g = GCR(D, prm)
    xs = [Field((n,)).set_zero() for _ in short]
    g.solve_queue([Field((n,), bs[0])] * 3, xs, width=2, ks=short)
    for s in range(3):
        assert g.last_iterations[s] == full_refs[s][0] and np.array_equal(g.last_history[s], full_refs[s][1])
        assert np.array_equal(xs[s].to_numpy(), full_refs[s][2])
    run_queue("sample", lad.ks[:4], bs[:4], refs[:4], 3, prm)           # another width and another number of systems
    run_queue("sample", lad.ks, bs, refs, 2, prm)


# ---- 9: the operator's own k ---------------------------------------------------------------------------------------------------------------
def test_the_operators_own_k_is_left_alone():
    lad, bs, _, refs = ladder_refs("sample")
    eo = evenodd("sample", "multi")
    n = eo.sizes()[0]
    prm = param(lad.restart, lad.max_iter, lad.tol)
    own = 0.12 + 0.01j
    eo.set_k(own)
    try:
        want = single("sample", own, bs[0], lad.restart, lad.max_iter, lad.tol)
        x = Field((n,)).set_zero()
        eo.solve(Field((n,), bs[0]), x, prm)
        first = (eo.last_iterations, eo.last_history.copy(), x.to_numpy())
        run_queue("sample", lad.ks, bs, refs, 2, prm)
        x = Field((n,)).set_zero()
        eo.solve(Field((n,), bs[0]), x, prm)
        for got in (first, (eo.last_iterations, eo.last_history, x.to_numpy())):
            assert got[0] == want[0] and np.array_equal(got[1], want[2]) and np.array_equal(got[2], want[3])
    finally:
        eo.set_k(emc.case_k("sample"))


# ---- 10: counters --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 3, 6])
def test_counters_follow_the_schedule(width):
    """lockstep steps and admissions are those of the schedule's model (tests/queue_cases.py) fed with the SINGLE solves' counts;
    max_iter and check_every are multiples of the cycle length, where the model is valid"""
    lad, bs, _, refs = ladder_refs("sample_longest_first")
    its = [r[0] for r in refs]
    steps, admissions = run_queue(lad.case, lad.ks, bs, refs, width, param(lad.restart, lad.max_iter, lad.tol, check_every=5))
    assert steps == qc.lockstep_steps(its, width, lad.restart), (steps, its)
    assert admissions == len(its) - min(width, len(its))
    if width < len(its):
        assert steps < qc.wait_for_group_steps(its, width, lad.restart)


# ---- 11: errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_every_x_untouched():
    lib = _lib.lib()
    c, m = ec.case("open4d"), ec.case_plan("open4d")        # n_e != n_o
    eo = evenodd("open4d", "multi")
    n, ne = c.n, m.even.size
    bs = [Field((n,), ec.rhs(n, 1 + s)) for s in range(3)]
    xs = [Field((n,), ec.rhs(n, 20 + s)) for s in range(3)]
    ref = [f.to_numpy() for f in xs + bs]
    ks = eq.spread("open4d", 3)
    prm = GCR_Param(0, 5, 10, 1e-8, False)

    def code(fn):
        with pytest.raises(MgcrError) as e:
            fn()
        return e.value.code, str(e.value)

    names = ("eo_queue_solves", "eo_queue_steps", "eo_queue_admissions")
    before = [stat(s) for s in names]
    # not an EvenOddDiracOp
    D = sparse("open4d")
    pc = prm._c()
    kv = np.ascontiguousarray(np.asarray(ks, np.complex128).view(np.float64).reshape(-1, 2))
    kp = kv.ctypes.data_as(C.POINTER(C.c_double))
    bh, xh = (C.c_void_p * 3)(*[f.h for f in bs]), (C.c_void_p * 3)(*[f.h for f in xs])
    for other in (MultiEvenOddDiracOp(eo, ks), D, DiracOp(D, 0.1)):
        assert lib.mgcr_eo_solve_queue(other.h, C.byref(pc), 2, 3, bh, xh, kp, None, 0, None, None) == 1, type(other)
    assert code(lambda: eo.solve_queue(bs, xs, [ks[0], 0.0, ks[2]], prm, width=2)) == (1, code(lambda: MultiEvenOddDiracOp(eo, [ks[0], 0.0, ks[2]]))[1]
                                                                                         .replace("mgcr_eo_multi_create", "mgcr_eo_solve_queue"))
    assert code(lambda: eo.solve_queue(bs, xs, None, prm, width=2))[0] == 1                               # k_ri == NULL
    assert code(lambda: eo.solve_queue(bs, xs, ks, prm, width=0))[0] == 1
    assert code(lambda: eo.solve_queue(bs, xs, ks, prm, width=17))[0] == 1
    assert code(lambda: eo.solve_queue([], [], [], prm, width=2))[0] == 1                                 # nsys = 0
    assert lib.mgcr_eo_solve_queue(eo.h, C.byref(pc), 2, 3, bh, (C.c_void_p * 3)(xs[0].h, None, xs[2].h), kp, None, 0, None, None) == 1   # a null handle
    assert lib.mgcr_eo_solve_queue(eo.h, C.byref(pc), 2, 3, None, xh, kp, None, 0, None, None) == 1
    assert lib.mgcr_eo_solve_queue(eo.h, None, 2, 3, bh, xh, kp, None, 0, None, None) == 1
    c1, msg = code(lambda: eo.solve_queue(bs, xs[:2] + [Field((ne,)).set_zero()], ks, prm, width=2))   # a Field of the even half
    assert c1 == 1 and "even half" in msg, msg
    assert code(lambda: eo.solve_queue(bs[:2] + [Field((n + 1,)).set_zero()], xs, ks, prm, width=2))[0] == 1
    assert code(lambda: eo.solve_queue(bs, [xs[0], xs[1], xs[0]], ks, prm, width=2))[0] == 1              # a repeated x
    assert code(lambda: eo.solve_queue(bs, [xs[0], bs[2], xs[2]], ks, prm, width=2))[0] == 1              # an x among the right-hand sides
    # the parameter cases mgcr_eo_multi_solve refuses
    inner = GCR(DiracOp(D, 0.1), GCR_Param(0, 5, 2, 1e-8, False))
    for bad in (GCR_Param(4, 0, 10, 1e-8, False), GCR_Param(0, 0, 10, 1e-8, False), GCR_Param(0, 17, 100, 1e-8, False),
                GCR_Param(0, 5, 10, 1e-8, False, solver_l=inner), GCR_Param(0, 5, 10, 1e-8, False, solver_r=inner),
                GCR_Param(0, 5, 10, 1e-8, False, solver_r=inner, flexible=True), GCR_Param(0, 5, 10, 1e-8, False, flexible=True)):
        assert code(lambda: eo.solve_queue(bs, xs, ks, bad, width=2))[0] == 7
    pp = prm._c()
    pp.profile_spmv = 1
    assert lib.mgcr_eo_solve_queue(eo.h, C.byref(pp), 2, 3, bh, xh, kp, None, 0, None, None) == 7
    # nothing was enqueued or touched
    assert all(np.array_equal(f.to_numpy(), r) for f, r in zip(xs + bs, ref))
    assert [stat(s) for s in names] == before
    # mgcr_gcr_solve_queue goes on refusing the operator
    fe = [Field((ne,)).set_zero() for _ in range(2)]
    c7, msg = code(lambda: GCR(eo, prm).solve_queue([fe[0]], [fe[1]], width=1))
    assert c7 == 7 and "even-odd" in msg
    eo.solve_queue(bs, xs, ks, GCR_Param(0, 5, 10, 0.0, False), width=8)                                  # width > nsys is allowed
    assert [stat(s) for s in names] == [before[0] + 1, before[1] + 10, before[2]]


# ---- 12: the experiment --------------------------------------------------------------------------------------------------------------------
def test_kcritical_evenodd_queue_equals_kcritical_evenodd(sample_matrix_path, capsys):
    import os
    D = read_data(os.path.basename(sample_matrix_path), directory=os.path.dirname(sample_matrix_path))
    capsys.readouterr()
    kw = dict(steps=4, max_iter=400, tol=1e-10)
    one = experiments.test_kcritical_evenodd(D, experiments.DIMS_4x4, 0.20611, 0.05, **kw)
    printed_one = capsys.readouterr().out
    queued = experiments.test_kcritical_evenodd_queue(D, experiments.DIMS_4x4, 0.20611, 0.05, width=2, **kw)
    printed_queued = capsys.readouterr().out
    assert len(queued) == 4 and queued == one
    assert printed_queued == printed_one and printed_one.count("\n") == 4
    assert len({t[1] for t in one}) > 1
