"""Hopping-parameter scans on the GPU: MultiDiracOp (1 - k_j D on column j of a block) through the k-wide apply and the batched GCR.
Everything is compared bit for bit (np.array_equal) with the single-Field entry points on DiracOp(D, ks[j]) — the two rules
include/mgcr.h states for mgcr_dirac_multi_create.  The shifts are distinct and partly complex: with equal shifts a wrong column
index would pass.  The scan's premise (where each column stops) is checked on the CPU in tests/test_kscan_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (DiracOp, Field, GCR, GCR_Param, MgcrError, MultiDiracOp, MultiField, Sparse, _lib, experiments,
                                     problems, read_data, set_option, stat)
from tests import kscan_cases as kc

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 8, 12, 16]


def shifts(k):
    return [0.05 + 0.01 * j + 0.02j * (j % 3) for j in range(k)]


def columns(n, k, seed0=0):
    return [Field((n,), problems.rhs_grid(n, seed0 + j)) for j in range(k)]


def poisson(n, patterns=True):
    prev = set_option("pattern_storage", 1 if patterns else 0)
    try:
        A = Sparse(*problems.poisson3d_csr(n))
    finally:
        set_option("pattern_storage", prev)
    return A, n ** 3


@pytest.fixture(scope="module")
def sample(sample_matrix_path):
    return read_data(os.path.basename(sample_matrix_path), directory=os.path.dirname(sample_matrix_path))


# ---- rule 1: the k-wide apply ---------------------------------------------------------------------------------------------
def check_apply(D, n, ks_list=KS):
    """column j of MultiDiracOp(D, ks)(X) == DiracOp(D, ks[j])(X_j), for every block width"""
    f = columns(n, max(ks_list))
    single = {}                       # (j, shift) -> the single apply's result: a column's shift does not depend on k
    for k in ks_list:
        ks = shifts(k)
        Y = MultiDiracOp(D, ks).apply_multi(MultiField.from_fields(f[:k])).to_numpy()
        for j in range(k):
            if j not in single:
                single[j] = DiracOp(D, ks[j])(f[j]).to_numpy()
            assert np.array_equal(Y[j], single[j]), (k, j)


IRREGULAR = [   # (rows, random_csr parameters, what the shape must reach)
    (257, dict(min_len=0, max_len=9), "slab"),                                   # plain slab, one lane per row, odd size
    (6000, dict(min_len=1, max_len=7, long_rows=7, long_len=3000), "long"),      # chunk rows and rows longer than a chunk
    (40000, dict(min_len=3, max_len=40), "tail"),                                # tail chunks with column windows (k = 12: 8 + 4)
    (700, dict(min_len=30, max_len=45), "lanes"),                                # several lanes per row
]


@pytest.mark.parametrize("n,kw,must", IRREGULAR, ids=[m for _, _, m in IRREGULAR])
def test_apply_irregular(n, kw, must):
    A = Sparse(n, n, *problems.random_csr(n, n, np.random.default_rng(n * 8), **kw))
    lay = A.ell_layout()
    assert A.storage_format()[0] == 0
    if must == "slab":
        assert lay["lanes"] == 1, lay
    if must in ("tail", "long"):
        assert lay["tail_rows"] > 0, lay
    if must == "long":
        assert kw["long_len"] > lay["tail_chunk_cap"] + lay["ell_width"], lay      # those rows do not fit a chunk
    if must == "lanes":
        assert lay["lanes"] > 1, lay
    check_apply(A, n)


def test_apply_real_slab():
    A, N = poisson(16, patterns=False)
    assert A.storage_format()[0] == 0
    check_apply(A, N)


def test_apply_stencil_view():
    A, N = poisson(64)
    assert A.storage_format()[0] == 3
    check_apply(A, N)


def test_apply_dictionary_with_values():
    prev = set_option("stencil_storage", 0)
    try:
        A, N = poisson(64)
    finally:
        set_option("stencil_storage", prev)
    assert A.storage_format()[0] == 1
    check_apply(A, N)


def test_apply_dictionary_of_columns():
    n = 40
    _, _, rowptr, col, val = problems.poisson3d_csr(n)
    val = val * (1.0 + np.random.default_rng(3).uniform(0, 1, val.size))
    B = Sparse(n ** 3, n ** 3, rowptr, col, val)
    assert B.storage_format()[0] == 2
    check_apply(B, n ** 3)


def test_apply_window_variant():
    N = 1 << 18
    A = Sparse(N, N, *problems.skewed_csr(N, np.random.default_rng(11), window=900, long_rows=3, long_len=2500))
    assert A.ell_layout()["x_window"] > 0
    check_apply(A, N)


def test_apply_sample(sample):
    assert sample.ell_layout()["lanes"] == 8
    check_apply(sample, sample.get_dim())


def test_queries_answer_for_the_sparse(sample):
    M = MultiDiracOp(sample, shifts(3))
    assert M.ncols == 3
    assert (M.get_dim(), M.get_nrow()) == (sample.get_dim(), sample.get_nrow())
    assert _lib.lib().mgcr_op_nnz(M.h) == _lib.lib().mgcr_op_nnz(sample.h)
    assert M.stored_bytes() == sample.stored_bytes() and M.storage_format() == sample.storage_format()
    assert M.ell_layout() == sample.ell_layout() and M.xr_fuse_kind() == sample.xr_fuse_kind()


# ---- rule 2: the batched solve --------------------------------------------------------------------------------------------
def check_solve(D, n, ks, param_args, rhs, x0=None, use_x0=False, M=None):
    """per column: history, iteration count, convergence flag and x == mgcr_gcr_solve with DiracOp(D, ks[j]) on that column"""
    k = len(ks)
    assert D.xr_fuse_kind() in (0, 1)          # the premise of the rule (include/mgcr.h)
    prm = GCR_Param(*param_args, False, use_x0=use_x0)
    g = GCR(M if M is not None else MultiDiracOp(D, ks), prm)
    X = MultiField.from_fields(x0) if x0 is not None else MultiField((n,), k).set_zero()
    g.solve_multi(MultiField.from_fields(rhs), X)
    Xh = X.to_numpy()
    single_its = []
    for j in range(k):
        x = x0[j].copy() if x0 is not None else Field((n,)).set_zero()
        gs = GCR(DiracOp(D, ks[j]), prm)
        gs.solve(rhs[j], x)
        single_its.append(gs.last_iterations)
        assert g.last_iterations[j] == gs.last_iterations, (j, g.last_iterations, gs.last_iterations)
        assert g.last_converged[j] == gs.last_converged, j
        assert np.array_equal(g.last_history[j], gs.last_history), j
        assert np.array_equal(Xh[j], x.to_numpy()), j
    return single_its


@pytest.mark.parametrize("use_x0", [False, True])
def test_scan_on_the_sample(sample, use_x0):
    n = sample.get_dim()
    b = Field((n,), problems.rhs_grid(n, kc.SCAN_RHS_SEED))
    x0 = [Field((n,), 0.01 * problems.rhs_grid(n, 7 + j)) for j in range(len(kc.SCAN_KS))] if use_x0 else None
    its = check_solve(sample, n, kc.SCAN_KS, (0, kc.SCAN_RESTART, kc.SCAN_MAX_ITER, kc.SCAN_TOL), [b] * len(kc.SCAN_KS), x0=x0, use_x0=use_x0)
    assert len(set(its)) >= 4, its                         # the columns were frozen at different steps ...
    assert its[-1] == kc.SCAN_MAX_ITER, its                # ... and k = 0.20 ran to the end


@pytest.mark.parametrize("args", [(0, 5, 40, 0.0), (0, 3, 200, 1e-8)])
@pytest.mark.parametrize("k", [4, 8])
def test_solve_poisson(args, k):
    A, N = poisson(32)
    check_solve(A, N, shifts(k), args, columns(N, k, 1))     # (the CPU oracle: some columns converge early, the others never; all finite)


def test_solve_small_system_takes_the_general_path():
    lib = _lib.lib()
    A, N = poisson(8)            # 512 rows: the single solve would run as one workgroup, in another summation order
    old = int(os.environ.get("MGCR_SMALL_SOLVE_ROWS", "1024"))
    lib.mgcr_set_small_solve_rows(0)
    try:
        check_solve(A, N, shifts(4), (0, 5, 60, 1e-10), columns(N, 4, 1))
    finally:
        lib.mgcr_set_small_solve_rows(old)


# ---- behaviour ------------------------------------------------------------------------------------------------------------
def test_set_k_between_two_solves(sample):
    n = sample.get_dim()
    rhs = columns(n, 3, 1)
    before = DiracOp(sample, 0.07)
    f = Field((n,), problems.rhs_grid(n, 9))
    y_before = before(f).to_numpy()
    M = MultiDiracOp(sample, [0.05, 0.08 + 0.02j, 0.11])
    args = (0, 5, 60, 1e-9)
    check_solve(sample, n, [0.05, 0.08 + 0.02j, 0.11], args, rhs, M=M)
    new = [0.12 - 0.03j, 0.06, 0.09 + 0.01j]
    M.set_k(new)
    check_solve(sample, n, new, args, rhs, M=M)
    Y = M.apply_multi(MultiField.from_fields(rhs)).to_numpy()
    for j in range(3):
        assert np.array_equal(Y[j], DiracOp(sample, new[j])(rhs[j]).to_numpy()), j
    # DiracOps on the same Sparse, made before and after, are not affected
    assert np.array_equal(before(f).to_numpy(), y_before)
    assert np.array_equal(DiracOp(sample, 0.07)(f).to_numpy(), y_before)


def test_errors_and_counter(sample):
    lib = _lib.lib()
    n = sample.get_dim()

    def code(fn):
        with pytest.raises(MgcrError) as e:
            fn()
        return e.value.code

    assert code(lambda: MultiDiracOp(sample, [])) == 1                       # k = 0
    assert code(lambda: MultiDiracOp(sample, [0.1] * 17)) == 1               # k = 17
    assert code(lambda: MultiDiracOp(sample, [0.1, 0.0, 0.2])) == 1          # a zero entry
    M = MultiDiracOp(sample, shifts(3))
    assert code(lambda: M.set_k([0.1, 0.0, 0.2])) == 1
    assert code(lambda: M.set_k([0.1, 0.2])) == 1
    B = MultiField.from_fields(columns(n, 3, 5))
    X = MultiField.from_fields(columns(n, 3))
    B2, X2 = MultiField.from_fields(columns(n, 2, 5)), MultiField.from_fields(columns(n, 2))
    ref, ref2 = X.to_numpy(), X2.to_numpy()
    f, y = Field((n,), problems.rhs_grid(n, 2)), Field((n,), problems.rhs_grid(n, 3))
    yref = y.to_numpy()
    prm = GCR_Param(0, 5, 10, 1e-8, False)
    # wrong block width
    assert code(lambda: M.apply_multi(B2, out=X2)) == 1
    assert code(lambda: GCR(M, prm).solve_multi(B2, X2)) == 1
    assert code(lambda: M.bench_apply_multi(B2, X2, 1)) == 1
    # the single-Field entry points
    assert code(lambda: M(f, out=y)) == 7
    assert code(lambda: M.bench_apply(f, y, 1)) == 7
    assert code(lambda: GCR(M, prm).solve(f, y)) == 7
    assert code(lambda: GCR(M, prm)(f, out=y)) == 7
    pc = prm._c()
    h = C.c_void_p()
    assert lib.mgcr_gcr_create(M.h, C.byref(pc), 1, C.byref(h)) == 7 and not h.value
    assert b"MultiDiracOp" in lib.mgcr_last_error()                          # the message says why
    assert lib.mgcr_gcr_solve(M.h, C.byref(pc), f.h, y.h, None, 0, None, None) == 7
    g = GCR(sample, prm)
    assert lib.mgcr_gcr_set_operator(g.h, M.h) == 7
    from mgpreconditionedgcr_amd._lib import MgParamC
    mp = MgParamC()
    assert lib.mgcr_mg_create(M.h, C.byref(mp), C.byref(h)) == 7 and not h.value
    assert np.array_equal(X.to_numpy(), ref) and np.array_equal(X2.to_numpy(), ref2) and np.array_equal(y.to_numpy(), yref)
    before = stat("multi_solves")
    GCR(M, prm).solve_multi(B, X)
    assert stat("multi_solves") == before + 1


# ---- the experiment -------------------------------------------------------------------------------------------------------
def test_kcritical_batched_equals_kcritical(sample, capsys):
    kw = dict(steps=4, max_iter=400, tol=1e-10)
    one = experiments.test_kcritical(sample, experiments.DIMS_4x4, 0.20611, 0.05, **kw)
    printed_one = capsys.readouterr().out
    batched = experiments.test_kcritical_batched(sample, experiments.DIMS_4x4, 0.20611, 0.05, **kw)
    printed_batched = capsys.readouterr().out
    assert len(batched) == 4 and batched == one          # k, iterations, convergence, last history entry (equal as floats)
    assert printed_batched == printed_one and printed_one.count("\n") == 4
    assert len({t[1] for t in one}) > 1                  # the ladder's columns stop at different steps
