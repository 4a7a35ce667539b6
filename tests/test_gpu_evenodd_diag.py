"""The even-odd Schur solve for operators with a site diagonal on the GPU (csrc/evenodd_diag.hip, mgcr_eo_create_diag), on the cases
of tests/evenodd_diag_cases.py.

The plan and the two coefficient arrays on the device equal the numpy model bit for bit.  The three bit rules of include/mgcr.h hold
with np.array_equal: Rule 1d — apply, prepare and the odd half of reconstruct equal the half operators of mgcr_eo_half_op with the
element-wise products formed on the host; Rule 2d — history, iteration count, flag and x of a GCR solve do not depend on the option
fused_apply; Rule 3d — a matrix without a diagonal gives exactly mgcr_eo_create's operator.  The counter evenodd_diag_fused_steps
moves on exactly the cases whose H_eo is stored one thread per row, evenodd_fused_steps never; every (MODE, WT) form of the fused
stage is reached.  mgcr_eo_solve solves the FULL system — the three premises of tests/test_evenodd_diag_cases.py, with the true
residual computed on the host — in fewer steps than GCR on the full operator.  Refusals come with their messages."""
import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, EvenOddDiagDiracOp, EvenOddDiracOp, EvenOddSparse, Field, GCR, GCR_Param, MgcrError,
                                     MultiEvenOddDiracOp, Sparse, _lib, set_option, stat)
from tests import evenodd_cases as ec
from tests import evenodd_diag_cases as dc

pytestmark = pytest.mark.gpu

KS = {"real": 0.13, "complex": 0.11 + 0.04j}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_operators():
    yield
    _cache.clear()


def sparse_of(c):
    return Sparse(c.n, c.n, c.rowptr, c.col, c.val)


def sparse(name):
    if ("M", name) not in _cache:
        _cache[("M", name)] = sparse_of(dc.case(name))
    return _cache[("M", name)]


def make(c, mat=None):
    mat = sparse_of(c) if mat is None else mat
    return EvenOddSparse(mat) if c.form == "matrix" else EvenOddDiagDiracOp(mat, c.k)


def evenodd(name, k=None):
    """The operator of case `name` (Dirac form: at k, default the case's own)"""
    c = dc.case(name) if k is None else dc.with_k(dc.case(name), k)
    key = ("eo", name, None if c.form == "matrix" else complex(c.k))
    if key not in _cache:
        _cache[key] = make(c, sparse(name))
    return _cache[key]


def field(v):
    return Field((v.size,), v)


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


def one_thread_per_row(eo):
    lay = eo.halves()[0].ell_layout()
    return lay["lanes"] == 1 and lay["tail_rows"] == 0


def code_of(fn):
    with pytest.raises(MgcrError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- 1. the plan and the coefficients on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.ALL)
def test_plan_split_merge_and_diag(name):
    c, m, co = dc.model(name)
    eo = evenodd(name)
    assert eo.sizes() == (c.n, m.even.size, m.odd.size)
    assert eo.get_dim() == eo.get_nrow() == m.even.size
    assert _lib.lib().mgcr_op_nnz(eo.h) == c.col.size                   # the whole matrix, diagonal included
    assert np.array_equal(eo.parity(), m.parity)
    a, inv = eo.diag()
    assert np.array_equal(bits(a), bits(co.a[m.even]))                   # a = (1, 0) - k d / d ...
    assert np.array_equal(bits(inv), bits(dc.einv(co.a[m.odd])))         # ... and 1 / a = (ar / den, -ai / den), bit for bit
    full = ec.rhs(c.n, 21)
    e, o = eo.split(field(full))
    assert np.array_equal(e.to_numpy(), full[m.even]) and np.array_equal(o.to_numpy(), full[m.odd])
    assert np.array_equal(eo.merge(e, o).to_numpy(), full)
    d_eo, d_oe = eo.halves()                                             # the OFF-DIAGONAL halves
    assert (d_eo.get_nrow(), d_eo.get_dim()) == (m.even.size, m.odd.size) and (d_oe.get_nrow(), d_oe.get_dim()) == (m.odd.size, m.even.size)
    assert _lib.lib().mgcr_op_nnz(d_eo.h) + _lib.lib().mgcr_op_nnz(d_oe.h) == c.col.size - dc.strip(name)[2]


def test_diag_of_an_operator_without_a_diagonal_is_all_ones():
    c, m = ec.case("chain"), ec.case_plan("chain")
    plain = EvenOddDiracOp(sparse_of(c), 0.1)
    a, inv = EvenOddDiagDiracOp.diag(plain)
    assert np.array_equal(a, np.ones(m.even.size)) and np.array_equal(inv, np.ones(m.odd.size))


# ---- 2. Rule 1d ----------------------------------------------------------------------------------------------------------------------
def rule1_params():
    out = []
    for name in dc.ALL:
        if dc.case(name).form == "matrix" or name in ("sample_twisted", "chain_zero_even"):     # no k, or a k the case is about
            out.append((name, None))
        else:
            out += [(name, "real"), (name, "complex")]
    return out


@pytest.mark.parametrize("name,kid", rule1_params())
def test_rule1d_apply_prepare_reconstruct(name, kid):
    k = None if kid is None else KS[kid]
    c, m, co = dc.model(name, k)
    eo = evenodd(name, k)
    h_eo, h_oe = eo.halves()
    print("storage of %s: H_eo format %r lanes %d, H_oe format %r lanes %d" % (name, h_eo.storage_format(), h_eo.ell_layout()["lanes"],
                                                                             h_oe.storage_format(), h_oe.ell_layout()["lanes"]))
    a, inv = eo.diag()
    xv = ec.rhs(m.even.size, 31)
    x = field(xv)
    y = eo(x).to_numpy()
    u = h_oe(x).to_numpy()
    v = h_eo(field(dc.emul(inv, u))).to_numpy()
    assert np.array_equal(y, dc.emul(a, xv) - dc.scalar_times(co.c2, v))
    want = dc.schur_apply(m, co, xv)                                     # ... and it is the Schur complement: the model agrees to rounding
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    bv = ec.rhs(c.n, 32)
    b = field(bv)
    got = eo.prepare(b).to_numpy()
    assert np.array_equal(got, bv[m.even] - dc.scalar_times(co.cn, h_eo(field(dc.emul(inv, bv[m.odd]))).to_numpy()))
    want = dc.prepare(m, co, bv)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    xe = ec.rhs(m.even.size, 33)
    xf = eo.reconstruct(b, field(xe)).to_numpy()
    assert np.array_equal(xf[m.odd], dc.emul(inv, bv[m.odd] - dc.scalar_times(co.cn, h_oe(field(xe)).to_numpy())))
    assert np.array_equal(xf[m.even], xe)
    want = dc.reconstruct(m, co, bv, xe)
    assert np.abs(xf - want).max() <= 1e-12 * np.abs(want).max()


def test_a_zero_on_the_even_diagonal_is_applied():
    c, m, co = dc.model("chain_zero_even")
    a, _ = evenodd("chain_zero_even").diag()
    assert np.count_nonzero(a == 0) == 1 and a[m.index[4]] == 0


@pytest.mark.parametrize("name", list(dc.FUSED_FORMS))
def test_every_fused_form_is_reached(name):
    h_eo, _ = evenodd(name).halves()
    fmt, npat = h_eo.storage_format()
    lay = h_eo.ell_layout()
    mode, width = dc.FUSED_FORMS[name]
    assert lay["lanes"] == 1 and lay["tail_rows"] == 0, lay
    assert fmt == mode, (fmt, npat, lay)
    assert (npat if mode == 3 else lay["ell_width"]) == width, (fmt, npat, lay)


# ---- 3. Rule 2d ----------------------------------------------------------------------------------------------------------------------
CONFIGS = {   # name: (GCR_Param arguments, lean_cycles) — the configurations of tests/test_gpu_evenodd.py
    "lean1": (dict(re=1, max_it=14), 1),
    "lean5": (dict(re=5, max_it=14), 1),
    "lean12": (dict(re=12, max_it=30), 1),
    "classic5": (dict(re=5, max_it=14), 0),
    "trunc4": (dict(trunc=4, max_it=14), 1),
    "lean5_x0": (dict(re=5, max_it=14, use_x0=True), 1),
}
COUNTERS = ("evenodd_diag_fused_steps", "evenodd_fused_steps")


def solve_twice(eo, bhat, x0, args, lean):
    out = []
    for fused in (1, 0):
        prev = (set_option("fused_apply", fused), set_option("lean_cycles", lean))
        try:
            before = [stat(n) for n in COUNTERS]
            x = field(x0)
            g = GCR(eo, GCR_Param(tau=1e-12, verb=False, **args))
            g.solve(bhat, x)
            out.append((g.last_history, g.last_iterations, g.last_converged, x.to_numpy(), [stat(n) - b for n, b in zip(COUNTERS, before)]))
        finally:
            set_option("fused_apply", prev[0])
            set_option("lean_cycles", prev[1])
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["d_sample", "d_open4d"] + list(dc.FUSED))
def test_rule2d_fused_apply_on_and_off(name, config):
    m = dc.case_plan(name)
    args, lean = CONFIGS[config]
    eo = evenodd(name)
    bhat = field(ec.rhs(m.even.size, 41))
    x0 = ec.rhs(m.even.size, 42) if args.get("use_x0") else np.zeros(m.even.size, ec.c128)
    on, off = solve_twice(eo, bhat, x0, args, lean)
    assert on[1] == off[1] and on[2] == off[2], (on[1:3], off[1:3])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[3], off[3])
    assert on[1] >= 1 and np.isfinite(on[0]).all() and np.isfinite(on[3]).all()
    assert off[4] == [0, 0]                                         # fused_apply off: never a fused stage
    assert on[4][1] == 0                                            # the counter of operators WITHOUT a diagonal never moves
    fused = one_thread_per_row(eo)
    assert fused == (name in dc.FUSED)
    if fused:
        assert on[4][0] >= on[1] - 1, (on[4], on[1])                # every step but the solve's short last one
    else:
        assert on[4][0] == 0


# ---- 4. Rule 3d ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.PURE)
def test_rule3d_no_diagonal_is_the_plain_operator(name):
    c, m = ec.case(name), ec.case_plan(name)
    k = ec.case_k(name)
    D = sparse_of(c)
    ops = (EvenOddDiagDiracOp(D, k), EvenOddDiracOp(D, k))
    a, inv = ops[0].diag()
    assert np.array_equal(a, np.ones(m.even.size)) and np.array_equal(inv, np.ones(m.odd.size))
    x, b, xe = field(ec.rhs(m.even.size, 61)), field(ec.rhs(c.n, 62)), field(ec.rhs(m.even.size, 63))
    res = []
    for op in ops:
        sol = Field((c.n,)).set_zero()
        op.solve(b, sol, GCR_Param(0, 5, 60, 1e-10, False))
        res.append((op(x).to_numpy(), op.prepare(b).to_numpy(), op.reconstruct(b, xe).to_numpy(), op.last_history, sol.to_numpy(),
                    op.last_iterations, op.last_converged))
    for got, want in zip(res[0][:5], res[1][:5]):
        assert np.array_equal(got, want)
    assert res[0][5:] == res[1][5:]
    # ... and it carries no diagonal: the scans take it
    assert MultiEvenOddDiracOp(ops[0], [0.1, 0.2]).ncols == 2


# ---- 5. set_k ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_sample", "d_scalar"])
def test_set_k_equals_a_fresh_operator(name):
    c, m = dc.case(name), dc.case_plan(name)
    k_new = 0.8 * c.k * (1 + 0.1j)
    eo = EvenOddDiagDiracOp(sparse(name), 0.05)
    eo.set_k(k_new)
    fresh = EvenOddDiagDiracOp(sparse(name), k_new)
    for got, want in zip(eo.diag(), fresh.diag()):
        assert np.array_equal(bits(got), bits(want))
    x = field(ec.rhs(m.even.size, 61))
    assert np.array_equal(eo(x).to_numpy(), fresh(x).to_numpy())
    b = field(ec.rhs(c.n, 62))
    res = []
    for op in (eo, fresh):
        sol = Field((c.n,)).set_zero()
        op.solve(b, sol, GCR_Param(0, 5, 60, 1e-10, False))
        res.append((op.last_history, op.last_iterations, op.last_converged, sol.to_numpy()))
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][3], res[1][3])


# ---- 6. skip-awareness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_sample", "d_scalar", "poisson_box"])
def test_gcr_object_stops_where_the_solve_stops(name):
    m = dc.case_plan(name)
    eo = evenodd(name)
    bhat = field(ec.rhs(m.even.size, 51))
    param = GCR_Param(0, 5, 2000, 1e-10, False)
    x = Field((m.even.size,)).set_zero()
    g = GCR(eo, param)
    g.solve(bhat, x)
    assert g.last_converged and g.last_iterations < 500
    y = GCR(eo, param, x0_mode=1)(bhat)                              # every launch behind the stop must do nothing
    assert np.array_equal(y.to_numpy(), x.to_numpy())


# ---- 7. end to end against the full system -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SOLVABLE)
def test_solve_against_the_full_system(name):
    tol = 1e-10
    c, m, co = dc.model(name)
    bv = ec.rhs(c.n)
    b = field(bv)
    eo = evenodd(name)
    x = Field((c.n,)).set_zero()
    eo.solve(b, x, GCR_Param(0, 5, 4000, tol, False))
    assert eo.last_converged
    xv = x.to_numpy()
    r = dc.full_apply(c, xv) - bv                                    # on the host, in numpy
    bn = np.linalg.norm(bv)
    true = np.linalg.norm(r) / bn
    mapped = eo.last_history[-1] * np.linalg.norm(eo.prepare(b).to_numpy()) / bn
    odd = np.linalg.norm(r[m.odd]) / bn
    full_op = sparse(name) if c.form == "matrix" else DiracOp(sparse(name), c.k)
    xfull = Field((c.n,)).set_zero()
    g = GCR(full_op, GCR_Param(0, 5, 4000, tol, False))
    g.solve(b, xfull)
    print("%s: true residual %.6e, mapped %.6e (|difference| %.3e), odd half %.3e, iterations %d against %d" % (
        name, true, mapped, abs(true - mapped), odd, eo.last_iterations, g.last_iterations))
    assert abs(true - mapped) <= 1e-14
    assert odd <= 1e-14
    assert g.last_converged and eo.last_iterations < g.last_iterations


def test_as_a_preconditioner_slot():
    c, m, co = dc.model("d_scalar")
    eo = evenodd("d_scalar")
    bv = ec.rhs(m.even.size, 81)
    inner = GCR(eo, GCR_Param(0, 4, 2, 1e-16, False), x0_mode=1)
    x = Field((m.even.size,)).set_zero()
    g = GCR(eo, GCR_Param(0, 5, 300, 1e-10, False, solver_r=inner, flexible=True))
    g.solve(field(bv), x)
    assert g.last_converged
    r = dc.schur_apply(m, co, x.to_numpy()) - bv
    assert np.linalg.norm(r) / np.linalg.norm(bv) <= 1e-9


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_a_singular_odd_diagonal_is_invalid_and_names_the_row():
    bad, good, k_bad, row = dc.rejected("singular_odd")
    code, msg = code_of(lambda: make(bad))
    assert code == 1 and "odd row %d" % row in msg and "no inverse" in msg, msg
    eo = make(good)
    before = [v.copy() for v in eo.diag()]
    x = field(ec.rhs(eo.sizes()[1], 91))
    y = eo(x).to_numpy()
    code, msg = code_of(lambda: eo.set_k(k_bad))
    assert code == 1 and "odd row %d" % row in msg and "no inverse" in msg, msg
    for got, want in zip(eo.diag(), before):                         # a refused k leaves the operator at its previous k
        assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(eo(x).to_numpy(), y)
    code, msg = code_of(lambda: eo.set_k(0.0))
    assert code == 1 and "No k value" in msg
    assert code_of(lambda: EvenOddDiagDiracOp(sparse_of(good), 0.0))[0] == 1


def test_an_odd_cycle_is_still_refused_with_its_entry():
    c, (row, col) = dc.rejected("triangle")
    for build in (lambda: EvenOddDiagDiracOp(sparse_of(c), 0.1), lambda: EvenOddSparse(sparse_of(c))):
        code, msg = code_of(build)
        assert code == 1 and "row %d, column %d" % (row, col) in msg, msg


def test_a_wrong_caller_bit_is_refused():
    hop, par, (row, col) = ec.rejected("flipped")
    D = Sparse(hop.n, hop.n, *dc.with_diagonal(hop, np.arange(hop.n), np.full(hop.n, 0.5)))
    code, msg = code_of(lambda: EvenOddDiagDiracOp(D, 0.1, par))
    assert code == 1 and "row %d, column %d" % (row, col) in msg, msg


def test_set_k_on_the_matrix_form_is_invalid():
    eo = evenodd("poisson_box")
    code, msg = code_of(lambda: eo.set_k(0.1))
    assert code == 1 and "matrix form" in msg, msg


def test_the_plain_entry_point_goes_on_refusing_a_diagonal():
    c = dc.case("dup_diag")
    code, msg = code_of(lambda: EvenOddDiracOp(sparse_of(c), 0.1))
    assert code == 1 and "row 3, column 3" in msg and "diagonal" in msg, msg


def test_the_scans_refuse_an_operator_with_a_diagonal():
    c, m = dc.case("d_chain"), dc.case_plan("d_chain")
    eo = evenodd("d_chain")
    code, msg = code_of(lambda: MultiEvenOddDiracOp(eo, [0.1, 0.2]))
    assert code == 7 and "diagonal" in msg, msg
    p = GCR_Param(0, 5, 5, 1e-10, False)
    code, msg = code_of(lambda: eo.solve_queue([Field((c.n,)).set_zero()], [Field((c.n,)).set_zero()], [0.1], p, width=1))
    assert code == 7 and "diagonal" in msg, msg


def test_wrong_lengths_are_invalid():
    c, m = dc.case("d_open4d"), dc.case_plan("d_open4d")  # n_e != n_o: an odd-sized Field is a wrong length for the even half
    eo = evenodd("d_open4d")
    ne, no, n = m.even.size, m.odd.size, c.n
    assert ne != no
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
