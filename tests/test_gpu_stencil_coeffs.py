"""Every stencil solve path on seven DISTINCT coefficients (tests/stencil_coeff_cases.py), bit for bit against the oracle in device order.

The Poisson box has six equal off-diagonals: a kernel that pairs the right x with the wrong slot's coefficient, or the real part of one
slot with the imaginary part of another, gives the same bits on it, so neither the comparison with the oracle nor any "path A == path B"
test on Poisson can see it.  Here the operators are anisotropic and non-symmetric, real and complex; the kernels' eligibility rules do
not look at the values, so they run the very kernels of the headline — and every case asserts the observation that proves it (storage
format, counters, row-map premises).  tests/test_stencil_coeff_cases.py shows on the CPU that every one of the 15 slot swaps moves
h(1) by five orders of magnitude more than the loosest tolerance in the suite; here there is no tolerance at all: np.array_equal on the
stand-alone apply, the DiracOp apply, the history, the iteration count, the convergence flag and x.

The oracle's device-order model depends on the operator's layout only: one oracle solve per (shape, coefficients, parameters, model)
serves every option variant of a case.
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mgpreconditionedgcr_amd")
from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, MultiField, Sparse, problems  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (checker only)
from tests import stencil_coeff_cases as sc  # noqa: E402
from tests.test_gpu_bitwise import assert_bitwise, device_model, solve_both  # noqa: E402

COUNTERS = ("resident_solves", "step_build_launches", "step_pair_launches", "step_pair_late_launches", "step_apply_own_launches",
            "step_keep_wide_launches", "start_build_launches")
_ORACLE = {}      # (dims, coefficients, shifted, Solve, model) -> (x, history, iterations, converged) of the oracle, read-only


@pytest.fixture(scope="module", autouse=True)
def _init():
    mg.init()
    yield
    _ORACLE.clear()


@contextlib.contextmanager
def _options(pairs):
    prev = [(name, mg.set_option(name, value)) for name, value in pairs]
    try:
        yield
    finally:
        for name, value in reversed(prev):
            mg.set_option(name, value)


def _model_key(A):
    """what tests/test_gpu_bitwise.py device_model reads of the operator"""
    lay = A.ell_layout()
    return tuple(sorted(lay.items())) + (A.xr_fuse_kind(),)


def _params(solve):
    return (GCR_Param(solve.truncation, solve.restart, solve.max_iter, sc.TOL, False),
            orc.gcr_param(truncation=solve.truncation, restart=solve.restart, max_iter=solve.max_iter, tol=sc.TOL))


def _solve_checked(tag, path, A, Ao, key, N, dims, solve, b, converges=True):
    """one GPU solve, compared with the oracle in device order (computed once per key); returns (what each counter rose by, the
    solver, x)"""
    gp, po = _params(solve)
    k = key + (solve, _model_key(A))
    before = {c: mg.stat(c) for c in COUNTERS}
    if k not in _ORACLE:
        gcr, x, ref, small = solve_both(A, Ao, N, gp, po, b, dims=dims)
        ref[0].setflags(write=False)
        ref[1].setflags(write=False)
        _ORACLE[k] = ref
    else:
        gcr = GCR(A, gp)
        x = Field(dims).set_zero()
        s0 = mg.stat("small_solves")
        gcr.solve(Field(dims, b), x)
        small = mg.stat("small_solves") > s0
    rose = {c: mg.stat(c) - before[c] for c in COUNTERS}
    assert not small
    assert_bitwise(tag, path, gcr, _ORACLE[k], None, x)
    assert gcr.last_iterations == solve.max_iter and np.isfinite(gcr.last_history).all()
    assert not converges or gcr.last_history[-1] < gcr.last_history[0]
    return rose, gcr, x


def _check_counters(what, wanted, rose):
    for name, rel in wanted:
        if rel == "print":
            print(what, name, rose[name])
        else:
            ok = {">0": rose[name] > 0, "==0": rose[name] == 0, "==1": rose[name] == 1}[rel]
            assert ok, "%s: %s rose by %d, wanted %s (all: %s)" % (what, name, rose[name], rel, rose)


def _check_applies(A, Ao, N, dims, xin):
    """the stand-alone apply and the DiracOp apply: the oracle's bits"""
    D, Do = DiracOp(A, sc.DIRAC_K), orc.dirac(Ao, sc.DIRAC_K)
    xf = Field(dims, xin)
    with device_model(A, N, False):
        assert np.array_equal(A(xf).to_numpy().ravel(), Ao(xin))
        assert np.array_equal(D(xf).to_numpy().ravel(), Do(xin))
    return D, Do


@pytest.mark.parametrize("case,which", sc.case_params(), ids=["%s-%s" % (c.id, w) for c, w in sc.case_params()])
def test_stencil_coefficients_bit_for_bit(case, which):
    nz, ny, nx = case.dims
    N, ncol, rowptr, col, val = sc.box_csr(nz, ny, nx, which)
    b, xin = problems.rhs_grid(N, sc.RHS_SEED), problems.rhs_grid(N, sc.X_SEED)
    Ao = orc.csr(N, ncol, rowptr, col, val)
    built = {}
    for v in case.variants:
        what = "%s-%s-%s" % (case.id, which, v.id)
        if v.build not in built:
            with _options(v.build):
                A = Sparse(N, ncol, rowptr, col, val)
            fmt = A.storage_format()
            assert fmt[0] == v.format[0] and v.format[1] in (None, fmt[1]), (what, fmt)
            if case.premise:       # the carried window, the plane-walk row map and the residual update inside the apply kernel
                assert A.xr_fuse_kind() == sc.XR_FUSE_KIND[which] and A.ell_layout()["reach"] == ny * nx, (what, A.xr_fuse_kind(), A.ell_layout())
                assert sc.row_map_premise(case.premise, case.dims, orc.row_map, orc.row_map_plane), what
            elif case.group == "window":
                print(what, "xr_fuse_kind", A.xr_fuse_kind(), "layout", A.ell_layout())
            built[v.build] = (A,) + _check_applies(A, Ao, N, case.dims, xin)
        A, D, Do = built[v.build]
        with _options(v.options):
            for solve in case.solves:
                tag = "coeffs_%s_%s_r%d_t%d_m%d" % (case.id, which, solve.restart, solve.truncation, solve.max_iter)
                rose, _, _ = _solve_checked(tag, v.id, A, Ao, (case.dims, which, False), N, case.dims, solve, b)
                _check_counters("%s %s" % (what, solve), v.counters, rose)
            for solve in v.dirac:
                tag = "coeffs_%s_%s_dirac_r%d_m%d" % (case.id, which, solve.restart, solve.max_iter)
                # (1 - k A with this k is far from the identity: the reference's recurrence does not reduce its residual here — the
                # history rises to about 3 over 12 steps, in the oracle as on the device; the bits are what is compared)
                rose, _, _ = _solve_checked(tag, v.id, D, Do, (case.dims, which, True), N, case.dims, solve, b, converges=False)
                _check_counters("%s DiracOp %s" % (what, solve), v.dirac_counters, rose)


# ---- the k-wide apply and the batched solve -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sc.BOTH)
@pytest.mark.parametrize("dims", sc.MULTI_APPLY_DIMS, ids=["%dx%dx%d" % d for d in sc.MULTI_APPLY_DIMS])
def test_apply_multi_columns_equal_the_oracle(dims, which):
    N, ncol, rowptr, col, val = sc.box_csr(*dims, which)
    A = Sparse(N, ncol, rowptr, col, val)
    assert A.storage_format() == (3, 7)
    Ao = orc.csr(N, ncol, rowptr, col, val)
    cols = [problems.rhs_grid(N, 20 + j) for j in range(max(sc.MULTI_APPLY_KS))]
    with device_model(A, N, False):
        refs = [Ao(c) for c in cols]
    for k in sc.MULTI_APPLY_KS:
        Y = A.apply_multi(MultiField.from_fields([Field((N,), c) for c in cols[:k]])).to_numpy()
        assert Y.shape == (k, N)
        for j in range(k):
            assert np.array_equal(Y[j], refs[j]), (k, j)


@pytest.mark.parametrize("which", sc.BOTH)
def test_solve_multi_columns_equal_the_single_solves(which):
    """column j of the batched solve == the single solve on column j == the oracle in device order"""
    dims, k, solve = sc.MULTI_SOLVE_DIMS, sc.MULTI_SOLVE_K, sc.MULTI_SOLVE
    N, ncol, rowptr, col, val = sc.box_csr(*dims, which)
    old = int(os.environ.get("MGCR_SMALL_SOLVE_ROWS", "1024"))      # (the library has no getter, tests/test_gpu_multi_rhs.py)
    mg.lib().mgcr_set_small_solve_rows(0)
    try:
        A = Sparse(N, ncol, rowptr, col, val)
        assert A.storage_format() == (3, 7)
        assert A.xr_fuse_kind() in (0, 1)      # the premise of the bit-for-bit rule (include/mgcr.h)
        Ao = orc.csr(N, ncol, rowptr, col, val)
        rhs = [problems.rhs_grid(N, 1 + j) for j in range(k)]
        gp, _ = _params(solve)
        g = GCR(A, gp)
        X = MultiField((N,), k).set_zero()
        before = mg.stat("multi_solves")
        g.solve_multi(MultiField.from_fields([Field((N,), c) for c in rhs]), X)
        assert mg.stat("multi_solves") == before + 1
        its, conv, hist, Xh = list(g.last_iterations), list(g.last_converged), [np.array(h) for h in g.last_history], X.to_numpy()
        for j in range(k):
            key = (dims, which, False, "column", j)
            _, gs, x = _solve_checked("coeffs_multi_%s_col%d" % (which, j), "single", A, Ao, key, N, (N,), solve, rhs[j])
            xo, ho, ito, co = _ORACLE[key + (solve, _model_key(A))]
            assert its[j] == gs.last_iterations == ito and conv[j] == gs.last_converged == co, j
            assert np.array_equal(hist[j], gs.last_history) and np.array_equal(hist[j], ho), j
            assert np.array_equal(Xh[j], x.to_numpy()) and np.array_equal(Xh[j], xo), j
    finally:
        mg.lib().mgcr_set_small_solve_rows(old)
