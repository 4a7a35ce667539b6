"""The low-precision GCR in even-odd form on the GPU (csrc/gcr32_eo.hip, mgcr_gcr32_create_eo) against the numpy model of
tests/gcr32_eo_cases.py.

Rule A — mgcr_gcr32_apply_matrix equals the model's fp32 Schur apply bit for bit on every case, and again after set_k where the
operator has a k; mgcr_gcr32_eo_diag has the bits of float32 of the fp64 operator's mgcr_eo_diag; mgcr_gcr32_eo_info equals the
model's plan.
Rule B — one apply twice gives the same bits; the step count of mgcr_gcr32_last equals the model's; with y64 the same algorithm in
fp64, |y_gpu - y64| <= 4 |y_model32 - y64| + 2^-40 |y64| (the bound of tests/test_gpu_gcr32.py, for the same reason: device and model
differ only in the order of fp64-accumulated sums).  A one-step solve has the model's bits.  One setting crosses two restart
boundaries at tol 0.
Rule C — mgcr_eo_solve with GCR(5), 1e-10, flexible and right_precond = the operator converges in the model's outer count (cases in
gcr32_eo_cases.SENSITIVE are recorded, not asserted) to a true Schur residual, formed on the host, <= 1e-10 (1 + 1e-3); the counters
move by the outer steps and max_iter times that; a GCR object solved twice gives the same bits; history, count and x_full are
bit-identical with fused_apply on and off.
Rule D — the refusals.
With MGCR_GCR32_EO_RECORD=<file> the measured Rule B ratios and the Rule C counts are written there;
tests/golden/observed_gcr32_eo.json is such a record."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (EvenOddBlockDiracOp, EvenOddDiagDiracOp, EvenOddDiracOp, EvenOddSparse, Field, GCR, GCR_Param,
                                     LowPrecisionEvenOddGCR, MgcrError, MultiEvenOddDiracOp, MultiField, Sparse, _lib, set_option, stat)
from tests import evenodd_diag_cases as dc
from tests import gcr32_cases as g
from tests import gcr32_eo_cases as e

pytestmark = pytest.mark.gpu

_cache = {}
_record = {"rule_b": {}, "rule_c": {}}
KEYS = [(name, k, inner) for name, k in e.all_cases() for inner in e.inner_settings(name, k)]


@pytest.fixture(scope="module", autouse=True)
def release_and_record():
    yield
    _cache.clear()
    path = os.environ.get("MGCR_GCR32_EO_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(_record, f, indent=1, sort_keys=True)


def sparse(name):
    if ("M", name) not in _cache:
        c = e.case(name)
        _cache[("M", name)] = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    return _cache[("M", name)]


def param(inner):
    return GCR_Param(0, inner[0], inner[1], inner[2], False)


def low(name, k, inner=e.INNER[0]):
    c = e.case(name, k)
    return LowPrecisionEvenOddGCR(sparse(name), c.k, param(inner), c.parity)


def outer_operator(name, k):
    """the fp64 even-odd operator of the case: mgcr_eo_create where nothing is stored on the diagonal, mgcr_eo_create_diag else"""
    c = e.case(name, k)
    if c.form == "matrix":
        return EvenOddSparse(sparse(name), c.parity)
    if e.plan_of(name).has_diag:
        return EvenOddDiagDiracOp(sparse(name), c.k, c.parity)
    return EvenOddDiracOp(sparse(name), c.k, c.parity)


def eo_diag64(A):
    """mgcr_eo_diag of any even-odd operator of the scalar forms: (a_even, 1 / a_odd) in complex128"""
    _, ne, no = A.sizes()
    a, inv = np.empty(ne, np.complex128), np.empty(no, np.complex128)
    _lib.check(_lib.lib().mgcr_eo_diag(A.h, a.ctypes.data, inv.ctypes.data))
    return a, inv


def field(v):
    return Field((v.size,), v)


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


def code_of(fn):
    with pytest.raises(MgcrError) as err:
        fn()
    return err.value.code, str(err.value)


def key_id(key):
    return "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1])


def expected_info(p):
    return dict(n=p.n, n_even=p.ne, n_odd=p.no, width_eo=p.hplans[0].W, width_oe=p.hplans[1].W, tail_rows_eo=p.hplans[0].tail_rows.size,
                tail_rows_oe=p.hplans[1].tail_rows.size, real_slab=p.real, has_diag=p.has_diag, stored_bytes=p.stored_bytes)


# ---- Rule A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(e.CASES))
def test_rule_a_apply_matrix_diag_and_info(name):
    p = e.plan_of(name)
    x = e.rhs(p.ne, 21)
    ks = [e.case(name, k).k for k in e.CASES[name]]
    op = low(name, ks[0])
    assert op.info() == expected_info(p)
    assert op.sizes() == (p.n, p.ne, p.no)
    assert op.get_dim() == op.get_nrow() == p.ne and _lib.lib().mgcr_op_nnz(op.h) == e.case(name).col.size
    m = e.EoModel(e.case(name, ks[0]))
    if ks[0] is not None:
        ks = ks + [0.2, -0.03 + 0.11j]
    for i, k in enumerate(ks):
        if i:
            op.set_k(k)
            m.set_k(k)
        assert np.array_equal(bits(op.apply_matrix(field(x)).to_numpy()), bits(m.apply_c128(x))), k
        a64, inv64 = eo_diag64(outer_operator(name, k))
        a32, inv32 = op.diag()
        assert np.array_equal(a32.view(np.uint32), e.to_c64(a64).view(np.uint32)), k
        assert np.array_equal(inv32.view(np.uint32), e.to_c64(inv64).view(np.uint32)), k
        if p.has_diag:
            co = e.coefficients(e.case(name, k), p)[1]
            assert np.array_equal(a32.view(np.uint32), co.a_even.view(np.uint32))
            assert np.array_equal(inv32.view(np.uint32), co.inv_a_odd.view(np.uint32))


def test_rule_a_a_workgroup_that_takes_a_second_tile():
    """n_e = 557 056: 544 tiles of 1024 rows for at most 512 workgroups"""
    c = e.case(e.BIG)
    p = e.plan_of(e.BIG)
    assert p.ne == 557056 and (p.ne + g.TILE - 1) // g.TILE == 544
    op = LowPrecisionEvenOddGCR(Sparse(c.n, c.n, c.rowptr, c.col, c.val), c.k, param(e.INNER[0]))
    assert op.info() == expected_info(p)
    x = e.rhs(p.ne, 21)
    assert np.array_equal(bits(op.apply_matrix(field(x)).to_numpy()), bits(e.EoModel(c).apply_c128(x)))


# ---- Rule B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_rule_b_inner_solve(key):
    name, k, inner = key
    c = e.case(name, k)
    f = e.rhs(e.plan_of(name).ne)
    op = low(name, k, inner)
    y1 = op(field(f)).to_numpy()
    last1 = op.last()
    y2 = op(field(f)).to_numpy()
    assert np.array_equal(bits(y1), bits(y2)) and op.last() == last1
    m32 = g.inner_solve(e.EoModel(c, e.f32), f, *inner)
    m64 = g.inner_solve(e.EoModel(c, e.f64), f, *inner)
    assert last1[0] == m32.n_iter == m64.n_iter
    assert abs(last1[1] - m32.rel) <= 1e-3 * m32.rel
    e_gpu, e_mod, scale = np.linalg.norm(y1 - m64.y), np.linalg.norm(m32.y - m64.y), np.linalg.norm(m64.y)
    print(key_id(key), "n_iter", last1[0], "|y_gpu - y64| / |y64| = %.3e, model %.3e, ratio %.3f" % (e_gpu / scale, e_mod / scale, e_gpu / e_mod))
    _record["rule_b"][key_id(key)] = dict(n_iter=last1[0], err_gpu=e_gpu / scale, err_model=e_mod / scale, ratio=e_gpu / e_mod,
                                          same_bits_as_model=bool(np.array_equal(bits(y1), bits(m32.y))))
    assert e_gpu <= 4 * e_mod + 2. ** -40 * scale


@pytest.mark.parametrize("name,k", e.all_cases())
def test_rule_b_one_step_has_the_models_bits(name, k):
    c = e.case(name, k)
    f = e.rhs(e.plan_of(name).ne)
    op = low(name, k, (1, 1, 0.))
    y = op(field(f)).to_numpy()
    m = g.inner_solve(e.EoModel(c), f, 1, 1, 0.)
    assert op.last()[0] == m.n_iter == 1
    assert np.array_equal(bits(y), bits(m.y))


@pytest.mark.parametrize("name", ["chain", "sample", "box_small", "bip_long"])
def test_a_zero_right_hand_side_gives_zero(name):
    ne = e.plan_of(name).ne
    op = low(name, "own")
    out = Field((ne,), e.rhs(ne, 3))                                  # whatever it held is overwritten
    y = op(Field((ne,)).set_zero(), out).to_numpy()
    assert not np.isnan(y.view(np.float64)).any() and np.array_equal(bits(y), bits(np.zeros(ne, np.complex128)))
    assert op.last() == (0, 0.0)
    assert np.array_equal(bits(op.apply_matrix(Field((ne,)).set_zero()).to_numpy()), bits(np.zeros(ne, np.complex128)))


# ---- Rule C ------------------------------------------------------------------------------------------------------------------------
def eo_solve(A, pc, b, n):
    bf, x = field(b), Field((n,)).set_zero()
    cap = pc.max_iter + 1
    hist = np.zeros(cap, np.float64)
    it, conv = C.c_int32(), C.c_int32()
    cc = pc._c()
    _lib.check(_lib.lib().mgcr_eo_solve(A.h, C.byref(cc), bf.h, x.h, hist.ctypes.data, cap, C.byref(it), C.byref(conv)))
    return x.to_numpy(), it.value, conv.value, hist[: it.value + 1].copy()


@pytest.mark.parametrize("key", [k for k in KEYS if k[2][2] > 0.], ids=key_id)
def test_rule_c_mixed_solve_through_mgcr_eo_solve(key):
    name, k, inner = key
    c = e.case(name, k)
    mod = e.mixed(name, c.k, inner, "f32")
    b = e.rhs_full(c)
    p, co = e.dplan(c)
    A = outer_operator(name, k)
    op = low(name, k, inner)
    outer = GCR_Param(0, e.OUTER["restart"], e.OUTER["max_iter"], e.OUTER["tol"], False, solver_r=op, flexible=True)
    before = stat("gcr32_applies"), stat("gcr32_steps")
    xs, it, conv, hist = eo_solve(A, outer, b, c.n)
    applies, steps = stat("gcr32_applies") - before[0], stat("gcr32_steps") - before[1]
    bh = dc.prepare(p, co, b)
    true_res = np.linalg.norm(bh - dc.schur_apply(p, co, xs[p.even])) / np.linalg.norm(bh)
    full_res = np.linalg.norm(b - dc.full_apply(dc.DCase(c.name, c.form, c.k, c.n, c.rowptr, c.col, c.val), xs)) / np.linalg.norm(b)
    print(key_id(key), "outer", it, "model", mod.n_iter, "true Schur residual %.3e" % true_res, "full %.3e" % full_res, "applies", applies,
          "steps", steps)
    _record["rule_c"][key_id(key)] = dict(outer=it, model_outer=mod.n_iter, model_inner_total=mod.inner_total, true_schur_residual=true_res,
                                          true_full_residual=full_res)
    assert conv == 1 and mod.converged
    if key not in e.SENSITIVE:
        assert it == mod.n_iter
    assert true_res <= 1e-10 * (1 + 1e-3)
    assert applies == it and steps == inner[1] * it
    # fused_apply on and off: history, count and x_full bit for bit
    prev = set_option("fused_apply", 0)
    try:
        xo, ito, convo, histo = eo_solve(A, outer, b, c.n)
    finally:
        set_option("fused_apply", prev)
    assert ito == it and convo == conv and np.array_equal(histo, hist) and np.array_equal(bits(xo), bits(xs))
    # through a GCR object on the even-odd operator, twice: the second solve has the first one's bits, and mgcr_gcr_solve agrees
    solver = GCR(A, outer)
    bhf = A.prepare(field(b))
    xa = solver.solve(bhf, Field((p.even.size,)).set_zero()).to_numpy()
    first = solver.last_iterations, solver.last_history.copy()
    xb = solver.solve(bhf, Field((p.even.size,)).set_zero()).to_numpy()
    assert np.array_equal(bits(xa), bits(xb)) and np.array_equal(bits(xa), bits(xs[p.even]))
    assert solver.last_iterations == first[0] == it and np.array_equal(solver.last_history, first[1])
    xc = Field((p.even.size,)).set_zero()
    cc = outer._c()
    itc = C.c_int32()
    _lib.check(_lib.lib().mgcr_gcr_solve(A.h, C.byref(cc), bhf.h, xc.h, None, 0, C.byref(itc), None))
    assert itc.value == it and np.array_equal(bits(xc.to_numpy()), bits(xa))


# ---- Rule D ------------------------------------------------------------------------------------------------------------------------
def test_rule_d_slots():
    c = e.case("chain")
    p = e.plan_of("chain")
    A = outer_operator("chain", "own")
    op = low("chain", "own")
    b, x = field(e.rhs(c.n)), Field((c.n,)).set_zero()

    def solve(pp, M=A):
        pc = pp._c()
        _lib.check(_lib.lib().mgcr_eo_solve(M.h, C.byref(pc), b.h, x.h, None, 0, None, None))

    for pp in (GCR_Param(0, 5, 50, 1e-10, False, solver_r=op),                         # flexible = 0
               GCR_Param(0, 5, 50, 1e-10, False, solver_l=op), GCR_Param(0, 5, 50, 1e-10, False, solver_l=op, flexible=True)):
        code, msg = code_of(lambda: solve(pp))
        assert code == 7 and "not a linear map" in msg, msg
        assert code_of(lambda: GCR(A, pp))[0] == 7
    good = GCR_Param(0, 5, 50, 1e-10, False, solver_r=op, flexible=True)
    solve(good)                                                                       # the accepted form
    # another colouring of the same matrix: every bit flipped is a valid two-colouring of the chain, with (n_e, n_o) = (22, 23) ...
    flipped = EvenOddDiracOp(sparse("chain"), c.k, (1 - p.parity).astype(np.int8))
    assert code_of(lambda: solve(good, flipped))[0] == 1                              # ... refused by the dimension already
    # ... and one of the SAME half sizes that differs in its colouring: two_parts' second component flipped
    t = e.case("two_parts")
    tp = e.plan_of("two_parts")
    par = tp.parity.copy()
    par[:6] ^= 1                                                                      # rows 0..5: a chain of 3 + 3, so n_e stays 8
    B = EvenOddDiracOp(sparse("two_parts"), t.k, par)
    assert B.sizes() == (tp.n, tp.ne, tp.no)
    opt = low("two_parts", "own")
    bt, xt = field(e.rhs(t.n)), Field((t.n,)).set_zero()
    pc = GCR_Param(0, 5, 50, 1e-10, False, solver_r=opt, flexible=True)._c()
    assert _lib.lib().mgcr_eo_solve(B.h, C.byref(pc), bt.h, xt.h, None, 0, None, None) == 1
    assert "colouring" in _lib.lib().mgcr_last_error().decode()
    assert code_of(lambda: GCR(B, GCR_Param(0, 5, 50, 1e-10, False, solver_r=opt, flexible=True)))[0] == 1
    # the same operator at another k is accepted: k is not compared
    other_k = EvenOddDiracOp(sparse("two_parts"), 0.5 * t.k)
    assert _lib.lib().mgcr_eo_solve(other_k.h, C.byref(pc), bt.h, xt.h, None, 0, None, None) == 0
    # an outer operator with site blocks
    blk = EvenOddBlockDiracOp(sparse("sample"), 0.15, 12)
    ops = low("sample", 0.15)
    bs, xs = field(e.rhs(3072)), Field((3072,)).set_zero()
    pcs = GCR_Param(0, 5, 50, 1e-10, False, solver_r=ops, flexible=True)._c()
    assert blk.get_dim() == ops.get_dim()
    assert _lib.lib().mgcr_eo_solve(blk.h, C.byref(pcs), bs.h, xs.h, None, 0, None, None) == 7
    assert "block" in _lib.lib().mgcr_last_error().decode()


def test_rule_d_entry_points():
    c = e.case("chain")
    p = e.plan_of("chain")
    op = low("chain", "own")
    code, msg = code_of(lambda: super(LowPrecisionEvenOddGCR, op).info())
    assert code == 7 and "mgcr_gcr32_eo_info" in msg, msg
    code, msg = code_of(lambda: low("box_small", None).set_k(0.1))                     # the matrix form has no k
    assert code == 1 and "matrix form" in msg
    wrong = field(e.rhs(p.ne + 1))
    assert code_of(lambda: op(wrong))[0] == 1
    assert code_of(lambda: op.apply_matrix(wrong))[0] == 1
    assert code_of(lambda: op.apply_matrix(field(e.rhs(c.n))))[0] == 1                  # a full-system Field
    L = _lib.lib()
    assert L.mgcr_gcr32_eo_info(sparse("chain").h, *([None] * 10)) == 1                  # not a low-precision GCR
    assert L.mgcr_gcr32_eo_diag(sparse("chain").h, None, None) == 1
    # the multi and queue solves refuse any preconditioner
    A = outer_operator("chain", "own")
    M = MultiEvenOddDiracOp(A, [c.k, 0.5 * c.k])
    X, Y = MultiField((c.n,), 2), MultiField((c.n,), 2)
    pc = GCR_Param(0, 5, 50, 1e-10, False, solver_r=op, flexible=True)._c()
    assert L.mgcr_eo_multi_solve(M.h, C.byref(pc), X.h, Y.h, None, 0, None, None) != 0
    b, x = field(e.rhs(c.n)), Field((c.n,)).set_zero()
    hs, xs = (C.c_void_p * 1)(b.h), (C.c_void_p * 1)(x.h)
    kk = (C.c_double * 2)(c.k, 0.)
    assert L.mgcr_eo_solve_queue(A.h, C.byref(pc), 1, 1, hs, xs, kk, None, 0, None, None) != 0
    plain = GCR_Param(0, 5, 50, 1e-10, False)._c()
    assert L.mgcr_eo_solve_queue(op.h, C.byref(plain), 1, 1, hs, xs, kk, None, 0, None, None) == 7
    assert code_of(lambda: GCR(op, GCR_Param(0, 5, 50, 1e-10, False)))[0] == 7


def test_rule_d_a_refused_set_k_leaves_the_operator_working():
    name = "d_scalar"
    c = e.case(name)
    f = e.rhs(e.plan_of(name).ne)
    op = low(name, "own")
    y0 = op(field(f)).to_numpy()
    d0 = op.diag()
    assert code_of(lambda: op.set_k(0.0))[0] == 1
    assert code_of(lambda: op.set_k(np.inf))[0] == 1
    assert code_of(lambda: op.set_k(1e30))[0] == 1                                       # c^2 overflows float
    d1 = op.diag()
    assert np.array_equal(d0[0].view(np.uint32), d1[0].view(np.uint32)) and np.array_equal(d0[1].view(np.uint32), d1[1].view(np.uint32))
    assert np.array_equal(bits(op(field(f)).to_numpy()), bits(y0)) and op.k == complex(c.k)


@pytest.mark.parametrize("name", e.REJECTED)
def test_refusals_at_creation_name_the_row(name):
    c, row, word = e.rejected(name)
    M = Sparse(c.n, c.n, c.rowptr, c.col, c.val)
    code, msg = code_of(lambda: LowPrecisionEvenOddGCR(M, c.k, param(e.INNER[0]), c.parity))
    assert code == 1 and ("row %d" % row) in msg and word in msg, msg


def test_refused_set_k_on_a_singular_odd_diagonal():
    good, k_bad, row = dc.rejected("singular_odd")[1:]
    M = Sparse(good.n, good.n, good.rowptr, good.col, good.val)
    op = LowPrecisionEvenOddGCR(M, good.k, param(e.INNER[0]))
    d0 = op.diag()
    code, msg = code_of(lambda: op.set_k(k_bad))
    assert code == 1 and ("row %d" % row) in msg and "no inverse" in msg, msg
    d1 = op.diag()
    assert np.array_equal(d0[1].view(np.uint32), d1[1].view(np.uint32)) and op.k == complex(good.k)
    code, msg = code_of(lambda: LowPrecisionEvenOddGCR(M, 0.0, param(e.INNER[0])))
    assert code == 1
    tri, (r, cc) = dc.rejected("triangle")
    code, msg = code_of(lambda: LowPrecisionEvenOddGCR(Sparse(tri.n, tri.n, tri.rowptr, tri.col, tri.val), tri.k, param(e.INNER[0])))
    assert code == 1 and ("entry (row %d, column %d)" % (r, cc)) in msg, msg
