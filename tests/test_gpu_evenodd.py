"""The even-odd preconditioned DiracOp on the GPU (csrc/evenodd.hip), on the cases of tests/evenodd_cases.py.

The plan on the device equals the numpy model.  The two bit rules of include/mgcr.h (mgcr_eo_create) hold with np.array_equal:
Rule 1 — apply, prepare and the odd half of reconstruct equal the half operators of mgcr_eo_half_op followed by mgcr_add_scaled;
Rule 2 — history, iteration count, flag and x of a GCR solve on the operator do not depend on the option fused_apply.  A GCR
object on the operator stops where the device-side flag says; mgcr_eo_set_k equals a fresh operator; and mgcr_eo_solve solves the
FULL system: the true residual of its solution, computed on the host, is the mapped last history entry, its odd half is rounding,
the solution is the full solve's to 10 tol, and the Schur solve takes fewer steps.

The storage form csr_build_device chose for both halves of every case is printed (format 0 slab, 1 / 2 dictionary, 3 stencil view;
lanes per row); the rules hold whatever came out.  Only the halves stored one thread per row — `chain`, `two_parts`, `scalar`,
`scalar_ti` and the one-unknown-per-site grids here — run the fused stage 2 (the counter evenodd_fused_steps moves); the others take
the plain applies either way.  test_every_fused_form_is_reached pins the storage those cases must come out in, so that Rule 2 runs
on every (MODE, WT) form the fused kernel is dispatched in: slab, value dictionary and column dictionary at a run-time width and at
the compiled-in width 7, the stencil view with 7 and with 9 kernel slots."""
import ctypes as C

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, EvenOddDiracOp, Field, GCR, GCR_Param, MgcrError, MultiField, Sparse, _lib, hostalg,
                                     set_option, stat)
from tests import evenodd_cases as ec

pytestmark = pytest.mark.gpu

KS = [0.13, 0.11 + 0.04j]       # real and complex
FUSED_CASES = ("chain", "two_parts", "scalar", "scalar_ti", "grid2d_const", "grid4d_const", "grid2d_varied", "w7_slab", "w7_ti",
               "w7_varied")     # D_eo stored one thread per row
# the form of schur_step_apply_kernel<MODE, WT, .> each of them must reach: (storage format = MODE, entries per row / stencil slots)
FUSED_FORMS = {"scalar": (0, 8), "w7_slab": (0, 7), "scalar_ti": (1, 8), "w7_ti": (1, 7), "grid2d_varied": (2, 4), "w7_varied": (2, 7),
               "grid2d_const": (3, 5), "grid4d_const": (3, 9)}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_operators():
    yield
    _cache.clear()


def sparse(name):
    if ("D", name) not in _cache:
        c = ec.case(name)
        _cache[("D", name)] = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    return _cache[("D", name)]


def evenodd(name, k):
    key = ("eo", name, complex(k))
    if key not in _cache:
        _cache[key] = EvenOddDiracOp(sparse(name), k)
    return _cache[key]


def field(v):
    return Field((v.size,), v)


def k_squared(k):
    return complex(hostalg.cmul(complex(k), complex(k)))


# ---- 1. the plan on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.ALL)
def test_plan_split_and_merge(name):
    c, m = ec.case(name), ec.case_plan(name)
    eo = evenodd(name, KS[0])
    assert eo.sizes() == (c.n, m.even.size, m.odd.size)
    assert eo.get_dim() == eo.get_nrow() == m.even.size
    assert _lib.lib().mgcr_op_nnz(eo.h) == c.col.size
    assert np.array_equal(eo.parity(), m.parity)
    full = ec.rhs(c.n, 21)
    e, o = eo.split(field(full))
    assert np.array_equal(e.to_numpy(), full[m.even]) and np.array_equal(o.to_numpy(), full[m.odd])
    assert np.array_equal(eo.merge(e, o).to_numpy(), full)                        # split, then merge: the identity, bit for bit
    ev, od = ec.rhs(m.even.size, 22), ec.rhs(m.odd.size, 23)
    merged = eo.merge(field(ev), field(od)).to_numpy()
    assert np.array_equal(merged[m.even], ev) and np.array_equal(merged[m.odd], od)   # every entry at its list index


# ---- 2. Rule 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS, ids=["real", "complex"])
@pytest.mark.parametrize("name", ec.ALL)
def test_rule1_apply_prepare_reconstruct(name, k):
    c, m = ec.case(name), ec.case_plan(name)
    eo = evenodd(name, k)
    d_eo, d_oe = eo.halves()
    print("storage of %s: D_eo format %r lanes %d, D_oe format %r lanes %d" % (name, d_eo.storage_format(), d_eo.ell_layout()["lanes"],
                                                                             d_oe.storage_format(), d_oe.ell_layout()["lanes"]))
    assert (d_eo.get_nrow(), d_eo.get_dim()) == (m.even.size, m.odd.size) and (d_oe.get_nrow(), d_oe.get_dim()) == (m.odd.size, m.even.size)
    x = field(ec.rhs(m.even.size, 31))
    y = eo(x)
    u = d_eo(d_oe(x))
    assert np.array_equal(y.to_numpy(), x.add_scaled(-k_squared(k), u).to_numpy())
    # ... and it is the Schur complement: the model agrees to rounding
    want = ec.schur_apply(m, k, x.to_numpy())
    assert np.abs(y.to_numpy() - want).max() <= 1e-12 * np.abs(want).max()
    b = field(ec.rhs(c.n, 32))
    be, bo = eo.split(b)
    assert np.array_equal(eo.prepare(b).to_numpy(), be.add_scaled(k, d_eo(bo)).to_numpy())
    xe = field(ec.rhs(m.even.size, 33))
    xf = eo.reconstruct(b, xe).to_numpy()
    assert np.array_equal(xf[m.odd], bo.add_scaled(k, d_oe(xe)).to_numpy())
    assert np.array_equal(xf[m.even], xe.to_numpy())


@pytest.mark.parametrize("name", list(FUSED_FORMS))
def test_every_fused_form_is_reached(name):
    d_eo, _ = evenodd(name, ec.case_k(name)).halves()
    fmt, npat = d_eo.storage_format()
    lay = d_eo.ell_layout()
    mode, width = FUSED_FORMS[name]
    assert lay["lanes"] == 1 and lay["tail_rows"] == 0, lay
    assert fmt == mode, (fmt, npat, lay)
    assert (npat if mode == 3 else lay["ell_width"]) == width, (fmt, npat, lay)      # stencil view: its slots (5 -> the 7-slot kernel)


# ---- 3. Rule 2 ----------------------------------------------------------------------------------------------------------------------
CONFIGS = {   # name: (GCR_Param arguments, lean_cycles)
    "lean1": (dict(re=1, max_it=14), 1),
    "lean5": (dict(re=5, max_it=14), 1),
    "lean12": (dict(re=12, max_it=30), 1),        # more directions than the fused kernels take: the chunked dot products run
    "classic5": (dict(re=5, max_it=14), 0),
    "trunc4": (dict(trunc=4, max_it=14), 1),
    "lean5_x0": (dict(re=5, max_it=14, use_x0=True), 1),
}


def solve_twice(eo, bhat, x0, args, lean):
    out = []
    for fused in (1, 0):
        prev = (set_option("fused_apply", fused), set_option("lean_cycles", lean))
        try:
            before = stat("evenodd_fused_steps")
            x = field(x0)
            g = GCR(eo, GCR_Param(tau=1e-12, verb=False, **args))
            g.solve(bhat, x)
            out.append((g.last_history, g.last_iterations, g.last_converged, x.to_numpy(), stat("evenodd_fused_steps") - before))
        finally:
            set_option("fused_apply", prev[0])
            set_option("lean_cycles", prev[1])
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["sample", "open4d", "periodic_ti"] + list(FUSED_CASES))
def test_rule2_fused_apply_on_and_off(name, config):
    m = ec.case_plan(name)
    args, lean = CONFIGS[config]
    eo = evenodd(name, ec.case_k(name))
    bhat = field(ec.rhs(m.even.size, 41))
    x0 = ec.rhs(m.even.size, 42) if args.get("use_x0") else np.zeros(m.even.size, ec.c128)
    on, off = solve_twice(eo, bhat, x0, args, lean)
    assert on[1] == off[1] and on[2] == off[2], (on[1:3], off[1:3])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[3], off[3])
    # (the reference's GCR takes its coefficients with the conjugate on the other side, src/GCR.h:230,258: on these random complex
    # operators a history may also grow — it must be the same history)
    assert on[1] >= 1 and np.isfinite(on[0]).all() and np.isfinite(on[3]).all()
    assert off[4] == 0                                              # fused_apply off: never the fused stage
    if name in FUSED_CASES:
        assert on[4] >= on[1] - 1, (on[4], on[1])                   # on: every step but the solve's short last one
    else:
        assert on[4] == 0
    if config == "lean12" and name in ("scalar", "scalar_ti"):
        assert on[1] > 11                                           # a cycle got past the 10 directions of the fused kernel


# ---- 4. skip-awareness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample", "scalar"])
def test_gcr_object_stops_where_the_solve_stops(name):
    m = ec.case_plan(name)
    eo = evenodd(name, ec.case_k(name))
    bhat = field(ec.rhs(m.even.size, 51))
    param = GCR_Param(0, 5, 2000, 1e-10, False)
    x = Field((m.even.size,)).set_zero()
    g = GCR(eo, param)
    g.solve(bhat, x)
    assert g.last_converged and g.last_iterations < 500              # max_iter is far above what the solve needs
    y = GCR(eo, param, x0_mode=1)(bhat)                              # every launch behind the stop must do nothing
    assert np.array_equal(y.to_numpy(), x.to_numpy())


# ---- 5. set_k ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample", "scalar"])
def test_set_k_equals_a_fresh_operator(name):
    m = ec.case_plan(name)
    k_new = 0.8 * ec.case_k(name) * (1 + 0.1j)
    eo = EvenOddDiracOp(sparse(name), 0.05)
    eo.set_k(k_new)
    fresh = EvenOddDiracOp(sparse(name), k_new)
    x = field(ec.rhs(m.even.size, 61))
    assert np.array_equal(eo(x).to_numpy(), fresh(x).to_numpy())
    b = field(ec.rhs(ec.case(name).n, 62))
    res = []
    for op in (eo, fresh):
        sol = Field((ec.case(name).n,)).set_zero()
        op.solve(b, sol, GCR_Param(0, 5, 60, 1e-10, False))
        res.append((op.last_history, op.last_iterations, op.last_converged, sol.to_numpy()))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][3], res[1][3])


# ---- 6. end to end against the full system -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.15, 0.18])
def test_solve_against_the_full_system(k):
    tol = 1e-10
    c, m = ec.case("sample"), ec.case_plan("sample")
    bv = ec.rhs(c.n)
    b = field(bv)
    eo = evenodd("sample", k)
    x = Field((c.n,)).set_zero()
    eo.solve(b, x, GCR_Param(0, 5, 4000, tol, False))
    assert eo.last_converged
    xv = x.to_numpy()
    r = ec.dirac_apply(c, k, xv) - bv                                # on the host, in numpy
    bhat = eo.prepare(b).to_numpy()
    true = np.linalg.norm(r) / np.linalg.norm(bv)
    mapped = eo.last_history[-1] * np.linalg.norm(bhat) / np.linalg.norm(bv)
    odd = np.linalg.norm(r[m.odd]) / np.linalg.norm(bv)
    xfull = Field((c.n,)).set_zero()
    g = GCR(DiracOp(sparse("sample"), k), GCR_Param(0, 5, 4000, tol, False))
    g.solve(b, xfull)
    err = np.linalg.norm(xv - xfull.to_numpy()) / np.linalg.norm(xfull.to_numpy())
    print("k = %g: true residual %.6e, mapped %.6e (ratio - 1 = %.3e), odd half %.3e, |x - x_full| / |x_full| = %.3e (%.2f tol), "
          "iterations %d against %d" % (k, true, mapped, true / mapped - 1, odd, err, err / tol, eo.last_iterations, g.last_iterations))
    assert abs(true / mapped - 1.0) <= 0.01
    assert odd <= 1e-13
    assert g.last_converged and err <= 10 * tol
    assert eo.last_iterations < g.last_iterations


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(MgcrError) as e:
        fn()
    return e.value.code, str(e.value)


def test_wrong_lengths_are_invalid():
    c, m = ec.case("open4d"), ec.case_plan("open4d")       # n_e != n_o: an odd-sized Field is a wrong length for the even half
    eo = evenodd("open4d", KS[0])
    ne, no, n = m.even.size, m.odd.size, c.n
    F = lambda size: Field((size,)).set_zero()             # noqa: E731
    p = GCR_Param(0, 5, 5, 1e-10, False)
    calls = [lambda: eo(F(no)), lambda: eo(F(ne), out=F(no)),
             lambda: eo.split(F(n - 1)), lambda: eo.split(F(n), F(no), F(no)), lambda: eo.split(F(n), F(ne), F(ne)),
             lambda: eo.merge(F(no), F(no)), lambda: eo.merge(F(ne), F(ne)), lambda: eo.merge(F(ne), F(no), F(n + 1)),
             lambda: eo.prepare(F(ne)), lambda: eo.prepare(F(n), F(no)),
             lambda: eo.reconstruct(F(ne), F(ne)), lambda: eo.reconstruct(F(n), F(no)), lambda: eo.reconstruct(F(n), F(ne), F(ne)),
             lambda: eo.solve(F(ne), F(n), p), lambda: eo.solve(F(n), F(ne), p),
             lambda: GCR(eo, p).solve(F(n), F(ne)), lambda: GCR(eo, p).solve(F(ne), F(no))]
    for i, call in enumerate(calls):
        assert code_of(call)[0] == 1, i


def test_zero_k_is_invalid():
    assert code_of(lambda: EvenOddDiracOp(sparse("chain"), 0.0))[0] == 1
    eo = EvenOddDiracOp(sparse("chain"), 0.1)
    code, msg = code_of(lambda: eo.set_k(0.0))
    assert code == 1 and "No k value" in msg


@pytest.mark.parametrize("name", ec.REJECTED)
def test_rejected_inputs_are_invalid_and_name_the_entry(name):
    c, parity, (row, col) = ec.rejected(name)
    D = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    code, msg = code_of(lambda: EvenOddDiracOp(D, 0.1, parity))
    assert code == 1 and "row %d, column %d" % (row, col) in msg, msg


def test_block_queue_and_multigrid_entry_points_refuse_it():
    m = ec.case_plan("chain")
    eo = evenodd("chain", KS[0])
    ne = m.even.size
    p = GCR_Param(0, 5, 5, 1e-10, False)
    X, Y = MultiField((ne,), 2).set_zero(), MultiField((ne,), 2).set_zero()
    assert code_of(lambda: eo.apply_multi(X, Y))[0] == 7
    assert code_of(lambda: GCR(eo, p).solve_multi(X, Y))[0] == 7
    assert code_of(lambda: GCR(eo, p).solve_queue([Field((ne,)).set_zero()], [Field((ne,)).set_zero()], width=1))[0] == 7
    h = C.c_void_p()
    assert _lib.lib().mgcr_mg_create(eo.h, C.byref(_lib.MgParamC()), C.byref(h)) == 7 and not h.value
    for query in (eo.storage_format, eo.ell_layout, eo.stored_bytes, eo.xr_fuse_kind):
        assert code_of(query)[0] == 7


def test_other_paths_counters_do_not_move():
    c = ec.case("chain")                                    # 23 even rows: small enough for the one-workgroup solve of a Sparse
    eo = evenodd("chain", ec.case_k("chain"))
    names = ("resident_solves", "small_solves", "step_build_launches", "start_build_launches", "multi_solves", "queue_solves")
    before = {k: stat(k) for k in names}
    x = Field((c.n,)).set_zero()
    eo.solve(field(ec.rhs(c.n, 71)), x, GCR_Param(0, 5, 200, 1e-10, False))
    assert eo.last_converged
    assert {k: stat(k) for k in names} == before


def test_as_a_preconditioner_slot():
    """GCR on the Schur operator, right-preconditioned by two sweeps of GCR(4) on the same operator (flexible): the nested use goes
    through the general path, and the solve still converges to the Schur system's solution"""
    m = ec.case_plan("scalar")
    k = ec.case_k("scalar")
    eo = evenodd("scalar", k)
    bv = ec.rhs(m.even.size, 81)
    inner = GCR(eo, GCR_Param(0, 4, 2, 1e-16, False), x0_mode=1)
    x = Field((m.even.size,)).set_zero()
    g = GCR(eo, GCR_Param(0, 5, 300, 1e-10, False, solver_r=inner, flexible=True))
    g.solve(field(bv), x)
    assert g.last_converged
    r = ec.schur_apply(m, k, x.to_numpy()) - bv
    assert np.linalg.norm(r) / np.linalg.norm(bv) <= 1e-9


def test_experiment_prints_and_returns_what_test_kcritical_does(capsys):
    from mgpreconditionedgcr_amd import experiments
    D = sparse("sample")
    out = experiments.test_kcritical_evenodd(D, ec.SAMPLE_DIMS, 0.20611, 0.10, steps=2, restart=5, max_iter=4000, tol=1e-10)
    lines = capsys.readouterr().out.splitlines()
    assert len(out) == len(lines) == 2
    for (k, its, conv, res), line, k_want in zip(out, lines, (0.10, 0.10 + (0.20611 - 0.10) / 2)):
        assert k == k_want and conv and res <= 1e-10 and 1 <= its < 4000
        assert line == "k = %f: converged after %d steps, residual %.10e" % (k, its, res)
        x = Field(ec.SAMPLE_DIMS).set_zero()
        eo = EvenOddDiracOp(D, k)
        eo.solve(Field(ec.SAMPLE_DIMS).fill_rhs(42), x, GCR_Param(0, 5, 4000, 1e-10, False, check_every=50))
        assert (eo.last_iterations, float(eo.last_history[-1])) == (its, res)       # set_k along the ladder = a fresh operator per k
