"""The low-precision GCR on the GPU (csrc/gcr32.hip, mgcr_gcr32_create) against the numpy model of tests/gcr32_cases.py.

Rule A — mgcr_gcr32_apply_matrix equals the model's fp32 apply bit for bit on every case, in both forms and after set_k.
Rule B — one apply twice gives the same bits; the step count of mgcr_gcr32_last equals the model's; with y64 the same algorithm in
fp64, |y_gpu - y64| <= 4 |y_model32 - y64| + 2^-40 |y64| (the device and the model differ only in the order of fp64-accumulated sums, so
their fp32 errors are of one size; the 4 leaves room for scalars that round one ulp apart).  A one-step solve is held to more: its
y = alpha f has the model's bits, since the two fp64 values of alpha differ by some 1e-15 relative and round to the same float unless
they straddle a rounding boundary (2^-24 apart: a chance of about 1e-8 per case; the inputs are fixed) — this is the check that
catches an alpha rounded before its division (tests/test_gcr32_cases.py).
Rule C — the mixed solve mgcr_gcr_solve(A64, GCR(5), 1e-10, flexible, right_precond = gcr32) converges in the model's number of outer
steps to a true residual <= 1e-10 (1 + 1e-3), the counters move by the outer steps and max_iter times that, and a GCR object
solved twice gives the same bits.  Rule D — the refusals.  Cases (g) (a value out of float's range) and (h) (f = 0).
The outer model is the library's fp64 GCR with the reference's conjugation (tests/gcr32_cases.py outer_solve).
The real operators (b, c) are solved for a real right-hand side there, the complex ones for a complex one (gcr32_cases.rhs_mixed has
the reason), and b and c once more for the complex one (test_rule_c_complex_data_on_the_real_operators).  A distributed outer
operator is refused on two ranks (tests/gcr32_dist_worker.py).
With MGCR_GCR32_RECORD=<file> the measured Rule B ratios and the Rule C counts (with those of the library's fp64 nested GCR in the
slot, recorded, not asserted) are written there; tests/golden/observed_gcr32.json is such a record."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, Field, GCR, GCR_Param, LowPrecisionGCR, MgcrError, MultiField, Sparse, _lib, stat)
from tests import gcr32_cases as g

pytestmark = pytest.mark.gpu

_cache = {}
_record = {"rule_b": {}, "rule_c": {}}
KEYS = [(name, k, inner) for name, k in g.all_cases() for inner in g.inner_settings(name)]


@pytest.fixture(scope="module", autouse=True)
def release_and_record():
    yield
    _cache.clear()
    path = os.environ.get("MGCR_GCR32_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(_record, f, indent=1, sort_keys=True)


def sparse(name):
    if ("M", name) not in _cache:
        n, rp, ci, va = g.matrix(name)
        _cache[("M", name)] = Sparse(n, n, rp, ci, va)
    return _cache[("M", name)]


def param(inner):
    return GCR_Param(0, inner[0], inner[1], inner[2], False)


def low(name, k, inner=g.INNER[0]):
    return LowPrecisionGCR(sparse(name), k, param(inner))


def field(v):
    return Field((v.size,), v)


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


def code_of(fn):
    with pytest.raises(MgcrError) as e:
        fn()
    return e.value.code, str(e.value)


def key_id(key):
    return "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1])


# ---- Rule A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(g.CASES))
def test_rule_a_apply_matrix_has_the_models_bits(name):
    x = g.rhs(g.matrix(name)[0], 21)
    k0 = g.CASES[name][0]
    for k in (k0, 0.07 - 0.02j if k0 is None else None):            # the case's own form, then the other one
        c = g.case(name, k)
        op = low(name, k)
        p = g.plan(c)
        assert op.info() == dict(n=c.n, ell_width=p.W, tail_rows=p.tail_rows.size, real_slab=p.real, stored_bytes=p.stored_bytes)
        assert op.get_dim() == op.get_nrow() == c.n and _lib.lib().mgcr_op_nnz(op.h) == c.col.size
        m = g.Model(c)
        assert np.array_equal(bits(op.apply_matrix(field(x)).to_numpy()), bits(m.apply_c128(x)))
        if k is not None:
            for k2 in (0.2, -0.03 + 0.11j):
                op.set_k(k2)
                m.set_k(k2)
                assert np.array_equal(bits(op.apply_matrix(field(x)).to_numpy()), bits(m.apply_c128(x)))


# ---- Rule B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_rule_b_inner_solve(key):
    name, k, inner = key
    c = g.case(name, k)
    f = g.rhs(c.n)
    op = low(name, k, inner)
    y1 = op(field(f)).to_numpy()
    last1 = op.last()
    y2 = op(field(f)).to_numpy()
    assert np.array_equal(bits(y1), bits(y2)) and op.last() == last1
    m32 = g.inner_solve(g.Model(c, g.f32), f, *inner)
    m64 = g.inner_solve(g.Model(c, g.f64), f, *inner)
    assert last1[0] == m32.n_iter == m64.n_iter
    assert abs(last1[1] - m32.rel) <= 1e-3 * m32.rel                # (the fp32 residual norms: far above fp32's floor at these tolerances)
    e_gpu, e_mod, scale = np.linalg.norm(y1 - m64.y), np.linalg.norm(m32.y - m64.y), np.linalg.norm(m64.y)
    print(key_id(key), "n_iter", last1[0], "|y_gpu - y64| / |y64| = %.3e, model %.3e, ratio %.3f" % (e_gpu / scale, e_mod / scale, e_gpu / e_mod))
    _record["rule_b"][key_id(key)] = dict(n_iter=last1[0], err_gpu=e_gpu / scale, err_model=e_mod / scale, ratio=e_gpu / e_mod,
                                          same_bits_as_model=bool(np.array_equal(bits(y1), bits(m32.y))))
    assert e_gpu <= 4 * e_mod + 2. ** -40 * scale


@pytest.mark.parametrize("name,k", g.all_cases())
def test_rule_b_one_step_has_the_models_bits(name, k):
    c = g.case(name, k)
    f = g.rhs(c.n)
    op = low(name, k, (1, 1, 0.))
    y = op(field(f)).to_numpy()
    m = g.inner_solve(g.Model(c), f, 1, 1, 0.)
    assert op.last()[0] == m.n_iter == 1
    assert np.array_equal(bits(y), bits(m.y))


# ---- Rule C ------------------------------------------------------------------------------------------------------------------------
def outer_operator(name, k):
    return sparse(name) if k is None else DiracOp(sparse(name), k)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_rule_c_mixed_solve(key):
    name, k, inner = key
    c = g.case(name, k)
    mod = g.mixed(name, k, inner, "f32")
    b = g.rhs_mixed(c)
    A = outer_operator(name, k)
    op = low(name, k, inner)
    outer = GCR_Param(0, g.OUTER["restart"], g.OUTER["max_iter"], g.OUTER["tol"], False, solver_r=op, flexible=True)
    pc = outer._c()
    bf, x = field(b), Field((c.n,)).set_zero()
    it, conv = C.c_int32(), C.c_int32()
    before = stat("gcr32_applies"), stat("gcr32_steps")
    _lib.check(_lib.lib().mgcr_gcr_solve(A.h, C.byref(pc), bf.h, x.h, None, 0, C.byref(it), C.byref(conv)))
    applies, steps = stat("gcr32_applies") - before[0], stat("gcr32_steps") - before[1]
    xs = x.to_numpy()
    ax, _ = g.apply_f64(c, xs)
    true_res = np.linalg.norm(b - ax) / np.linalg.norm(b)
    print(key_id(key), "outer", it.value, "model", mod.n_iter, "true residual %.3e" % true_res, "applies", applies, "steps", steps)
    assert conv.value == 1 and mod.converged
    assert it.value == mod.n_iter
    assert true_res <= 1e-10 * (1 + 1e-3)
    # the counters live on the device and count the applies that ran: the apply the outer solver enqueues behind its last residual
    # update is handed that solve's stopping test (Gcr32Gate) and does not run
    assert applies == it.value and steps == inner[1] * it.value
    # through a GCR object, twice: the second solve has the first one's bits
    solver = GCR(A, outer)
    xa = solver.solve(field(b), Field((c.n,)).set_zero()).to_numpy()
    first = solver.last_iterations, solver.last_history.copy()
    xb = solver.solve(field(b), Field((c.n,)).set_zero()).to_numpy()
    assert np.array_equal(bits(xa), bits(xb)) and np.array_equal(bits(xa), bits(xs))
    assert solver.last_iterations == first[0] == it.value and np.array_equal(solver.last_history, first[1])
    print(key_id(key), "history", " ".join("%.2e" % h for h in solver.last_history))
    # recorded, not asserted: the library's own fp64 nested GCR in the slot
    nested = GCR(A, param(inner))
    ref = GCR(A, GCR_Param(0, g.OUTER["restart"], g.OUTER["max_iter"], g.OUTER["tol"], False, solver_r=nested, flexible=True))
    ref.solve(field(b), Field((c.n,)).set_zero())
    _record["rule_c"][key_id(key)] = dict(outer=it.value, model_outer=mod.n_iter, model_inner_total=mod.inner_total, true_residual=true_res,
                                          fp64_nested_outer=ref.last_iterations, fp64_nested_converged=bool(ref.last_converged))


@pytest.mark.parametrize("key", g.COMPLEX_ON_REAL, ids=key_id)
def test_rule_c_complex_data_on_the_real_operators(key):
    """The full mixed solve with the COMPLEX right-hand side on the real slabs (b, c): convergence, the true residual and the
    counters on all four; the outer count equals the fp32 model's where that count is robust — on the two known exceptions
    (gcr32_cases.SENSITIVE), whose counts hang on rounding-size perturbations, it is recorded only."""
    name, k, inner = key
    c = g.case(name, k)
    mod = g.mixed(name, k, inner, "f32", True)
    b = g.rhs(c.n)
    A, op = outer_operator(name, k), low(name, k, inner)
    pc = GCR_Param(0, g.OUTER["restart"], g.OUTER["max_iter"], g.OUTER["tol"], False, solver_r=op, flexible=True)._c()
    bf, x = field(b), Field((c.n,)).set_zero()
    it, conv = C.c_int32(), C.c_int32()
    before = stat("gcr32_applies"), stat("gcr32_steps")
    _lib.check(_lib.lib().mgcr_gcr_solve(A.h, C.byref(pc), bf.h, x.h, None, 0, C.byref(it), C.byref(conv)))
    applies, steps = stat("gcr32_applies") - before[0], stat("gcr32_steps") - before[1]
    ax, _ = g.apply_f64(c, x.to_numpy())
    true_res = np.linalg.norm(b - ax) / np.linalg.norm(b)
    print(key_id(key), "complex rhs: outer", it.value, "model", mod.n_iter, "true residual %.3e" % true_res, "applies", applies, "steps", steps)
    _record["rule_c"]["complex-rhs-" + key_id(key)] = dict(outer=it.value, model_outer=mod.n_iter, true_residual=true_res)
    assert conv.value == 1 and mod.converged
    assert true_res <= 1e-10 * (1 + 1e-3)
    assert applies == it.value and steps == inner[1] * it.value
    if key not in g.SENSITIVE:
        assert it.value == mod.n_iter


# ---- Rule D ------------------------------------------------------------------------------------------------------------------------
def test_rule_d_inner_parameters():
    M = sparse("f")
    other = low("f", 0.45)
    for bad, word in ((GCR_Param(3, 0, 8, 0.1, False), "truncation"), (GCR_Param(0, 0, 8, 0.1, False), "restart"),
                      (GCR_Param(0, 17, 8, 0.1, False), "restart"), (GCR_Param(0, 8, 8, 0.1, False, solver_r=other), "preconditioner"),
                      (GCR_Param(0, 8, 8, 0.1, False, solver_l=other), "preconditioner"), (GCR_Param(0, 8, 8, 0.1, False, use_x0=True), "use_x0"),
                      (GCR_Param(0, 8, 8, 0.1, False, flexible=True), "flexible"), (GCR_Param(0, 8, 8, 0.1, False, profile_spmv=True), "profile_spmv")):
        code, msg = code_of(lambda: LowPrecisionGCR(M, 0.45, bad))
        assert code == 7 and word in msg, msg
        code, msg = code_of(lambda: other.set_param(bad))
        assert code == 7 and word in msg, msg
    assert code_of(lambda: LowPrecisionGCR(M, 0.45, GCR_Param(0, 8, 0, 0.1, False)))[0] == 1
    assert code_of(lambda: LowPrecisionGCR(M, 0.0, param(g.INNER[0])))[0] == 1                    # k = 0
    assert code_of(lambda: LowPrecisionGCR(M, 1e39, param(g.INNER[0])))[0] == 1                   # k out of float's range
    assert code_of(lambda: LowPrecisionGCR(M, complex(0.1, np.nan), param(g.INNER[0])))[0] == 1
    # a tol below fp32's reach is accepted and runs max_iter steps
    c = g.case("f")
    tiny = LowPrecisionGCR(M, c.k, GCR_Param(0, 4, 6, 1e-30, False))
    tiny(field(g.rhs(c.n)))
    assert tiny.last()[0] == 6


def test_rule_d_a_refused_set_k_or_set_param_leaves_the_operator_working():
    c = g.case("d")
    f = g.rhs(c.n)
    op = low("d", c.k)
    y0 = op(field(f)).to_numpy()
    assert code_of(lambda: op.set_k(0.0))[0] == 1
    assert code_of(lambda: op.set_k(np.inf))[0] == 1
    assert code_of(lambda: op.set_param(GCR_Param(0, 17, 8, 0.1, False)))[0] == 7
    assert code_of(lambda: op.set_param(GCR_Param(0, 8, 0, 0.1, False)))[0] == 1
    assert np.array_equal(bits(op(field(f)).to_numpy()), bits(y0))
    op.set_param(param(g.INNER[1]))                                  # an accepted one takes effect: more slots, more steps
    y1 = op(field(f)).to_numpy()
    m = g.inner_solve(g.Model(c), f, *g.INNER[1])
    assert op.last()[0] == m.n_iter and np.linalg.norm(y1 - m.y) <= 1e-4 * np.linalg.norm(m.y)
    code, msg = code_of(lambda: low("b", None).set_k(0.1))           # the matrix form has no k
    assert code == 1 and "matrix form" in msg


def test_rule_d_matrix_checks():
    inner = param(g.INNER[0])
    n, rp, ci, va = g.matrix("f")
    pc = inner._c()
    h = C.c_void_p()
    L = _lib.lib()
    bad_col = ci.copy()
    bad_col[3] = n
    assert L.mgcr_gcr32_create(n, rp.ctypes.data, bad_col.ctypes.data, va.ctypes.data, None, C.byref(pc), C.byref(h)) == 1 and not h.value
    bad_rp = rp.copy()
    bad_rp[2] = bad_rp[3] + 1
    assert L.mgcr_gcr32_create(n, bad_rp.ctypes.data, ci.ctypes.data, va.ctypes.data, None, C.byref(pc), C.byref(h)) == 1 and not h.value
    for name in ("mgcr_gcr32_set_k", "mgcr_gcr32_set_param", "mgcr_gcr32_info", "mgcr_gcr32_apply_matrix", "mgcr_gcr32_last"):
        args = {"mgcr_gcr32_set_k": (None,), "mgcr_gcr32_set_param": (C.byref(pc),), "mgcr_gcr32_info": (None,) * 5,
                "mgcr_gcr32_apply_matrix": (None, None), "mgcr_gcr32_last": (None, None)}[name]
        assert getattr(L, name)(sparse("f").h, *args) == 1, name                   # not a low-precision GCR


def test_rule_d_slots_and_entry_points():
    c = g.case("f")
    A = DiracOp(sparse("f"), c.k)
    op = low("f", c.k)
    b, x = field(g.rhs(c.n)), Field((c.n,)).set_zero()

    def solve(p, M=A):
        pc = p._c()
        _lib.check(_lib.lib().mgcr_gcr_solve(M.h, C.byref(pc), b.h, x.h, None, 0, None, None))

    for p in (GCR_Param(0, 5, 50, 1e-10, False, solver_r=op),                         # flexible = 0
              GCR_Param(0, 5, 50, 1e-10, False, solver_l=op), GCR_Param(0, 5, 50, 1e-10, False, solver_l=op, flexible=True)):
        code, msg = code_of(lambda: solve(p))
        assert code == 7 and "not a linear map" in msg, msg
        assert code_of(lambda: GCR(A, p))[0] == 7
    good = GCR_Param(0, 5, 50, 1e-10, False, solver_r=op, flexible=True)
    solver = GCR(A, GCR_Param(0, 5, 50, 1e-10, False))
    solver.param = GCR_Param(0, 5, 50, 1e-10, False, solver_r=op)                    # mgcr_gcr_set_param at solve time
    assert code_of(lambda: solver.solve(b, x))[0] == 7
    wrong = DiracOp(sparse("b"), 0.1)                                                # 315 rows against 45
    b2, x2 = field(g.rhs(315)), Field((315,)).set_zero()
    pc = good._c()
    assert _lib.lib().mgcr_gcr_solve(wrong.h, C.byref(pc), b2.h, x2.h, None, 0, None, None) == 1
    late = GCR(good)                                                                 # the operator comes later: checked then
    assert code_of(lambda: late.initialise(wrong))[0] == 1
    # as the system operator of a solve, in multigrid, on blocks, in the queues, in the storage queries
    plain = GCR_Param(0, 5, 50, 1e-10, False)
    assert code_of(lambda: solve(plain, op))[0] == 7
    assert code_of(lambda: GCR(op, plain))[0] == 7
    assert code_of(lambda: GCR(plain).initialise(op))[0] == 7
    X, Y = MultiField((c.n,), 2), MultiField((c.n,), 2)
    assert code_of(lambda: op.apply_multi(X, Y))[0] == 7
    pcp = plain._c()
    L = _lib.lib()
    assert L.mgcr_gcr_solve_multi(op.h, C.byref(pcp), X.h, Y.h, None, 0, None, None) == 7
    hs = (C.c_void_p * 1)(b.h)
    xs = (C.c_void_p * 1)(x.h)
    kk = (C.c_double * 2)(0.1, 0.)
    assert L.mgcr_gcr_solve_queue(op.h, C.byref(pcp), 1, 1, hs, xs, None, None, 0, None, None) == 7
    assert L.mgcr_eo_solve_queue(op.h, C.byref(pcp), 1, 1, hs, xs, kk, None, 0, None, None) == 7
    assert L.mgcr_mg_create(op.h, C.byref(_lib.MgParamC()), C.byref(C.c_void_p())) == 7
    for q in (op.stored_bytes, op.storage_format, op.ell_layout, op.xr_fuse_kind):
        assert code_of(q)[0] == 7
    assert L.mgcr_op_halo_kind(op.h, C.byref(C.c_int32())) == 7
    # Fields of the wrong length
    assert code_of(lambda: op(b2))[0] == 1
    assert code_of(lambda: op.apply_matrix(b2))[0] == 1


# ---- cases (g) and (h) ---------------------------------------------------------------------------------------------------------------
def test_case_g_a_value_out_of_floats_range_is_refused():
    n, rp, ci, va = g.matrix("g")
    M = Sparse(n, n, rp, ci, va)                                      # fp64 takes it
    for k in (0.09, None):
        code, msg = code_of(lambda: LowPrecisionGCR(M, k, param(g.INNER[0])))
        assert code == 1 and ("row %d " % g.G_ROW) in msg, msg


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_case_h_a_zero_right_hand_side_gives_zero(name):
    c = g.case(name)
    op = low(name, c.k)
    out = Field((c.n,), g.rhs(c.n, 3))                                # whatever it held is overwritten
    y = op(Field((c.n,)).set_zero(), out).to_numpy()
    assert not np.isnan(y.view(np.float64)).any() and np.array_equal(bits(y), bits(np.zeros(c.n, np.complex128)))
    assert op.last() == (0, 0.0)
    assert np.array_equal(bits(op.apply_matrix(Field((c.n,)).set_zero()).to_numpy()), bits(np.zeros(c.n, np.complex128)))


# ---- Rule D, a distributed outer operator: two ranks on the one GPU --------------------------------------------------------------------
def test_rule_d_a_distributed_outer_operator_is_refused(tmp_path):
    import socket
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    world = 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    logs = [open(str(tmp_path / ("rank%d.log" % r)), "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "gcr32_dist_worker.py"), str(r), str(world), str(port), str(tmp_path)],
                              env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    t0 = time.time()
    while any(p.poll() is None for p in procs):        # the first failing rank ends the run: the other would wait for it in a collective
        if any(p.poll() not in (None, 0) for p in procs) or time.time() - t0 > 200:
            for q in procs:
                if q.poll() is None:
                    q.kill()
            break
        time.sleep(0.05)
    for r, p in enumerate(procs):
        p.wait()
        logs[r].seek(0)
        assert p.returncode == 0, "rank %d: %s" % (r, logs[r].read()[-3000:])
    for r in range(world):
        res = json.load(open(str(tmp_path / ("rank%d.json" % r))))
        assert sorted(res) == ["create_dirac", "create_sparse", "set_operator", "solve_dirac", "solve_sparse"]
        for where, (code, msg) in res.items():
            assert code == 7 and "distributed" in msg, (r, where, code, msg)
