"""Blocks of k Fields on the GPU: pack / unpack, block BLAS-1, the k-wide apply and the batched GCR.  Everything is compared
bit for bit (np.array_equal) with the single-Field entry points on the same columns — the two rules of include/mgcr.h
(mgcr_op_apply_multi, mgcr_gcr_solve_multi).  The comparison of the batched solve with the CPU oracle in device summation order — cycle
lengths, ragged column groups, frozen columns, x0 through every apply form — is in tests/test_gpu_multi_rhs_edges.py (cases:
tests/multi_rhs_cases.py, their premises on the CPU: tests/test_multi_rhs_cases.py)."""
import os

import numpy as np
import pytest

from mgpreconditionedgcr_amd import (Dense, DiracOp, Field, GCR, GCR_Param, HierarchicalSparse, MgcrError, MultiField, Sparse, _lib,
                                     problems, read_data, set_option, stat)

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 8, 12, 16]


def columns(n, k, seed0=0):
    return [Field((n,), problems.rhs_grid(n, seed0 + j)) for j in range(k)]


def poisson(n, patterns=True):
    N = n ** 3
    prev = set_option("pattern_storage", 1 if patterns else 0)
    try:
        A = Sparse(*problems.poisson3d_csr(n))
    finally:
        set_option("pattern_storage", prev)
    return A, N


@pytest.fixture(scope="module")
def sample(sample_matrix_path):
    return read_data(os.path.basename(sample_matrix_path), directory=os.path.dirname(sample_matrix_path))


# ---- pack / unpack, BLAS-1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 65537, 1 << 21])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_pack_unpack_and_blas1(n, k):
    fa, fb = columns(n, k), columns(n, k, 100)
    A, B = MultiField.from_fields(fa), MultiField.from_fields(fb)
    host = A.to_numpy()
    assert host.shape == (k, n)
    for j in range(k):
        assert np.array_equal(host[j], fa[j].to_numpy())
        assert np.array_equal(A.column(j).to_numpy(), host[j])
    assert np.array_equal(MultiField((n,), k, host).to_numpy(), host)       # upload: host [k][n] -> device [n][k]
    d, nn = A.dot(B), A.squarednorm()
    for j in range(k):
        assert d[j] == fa[j].dot(fb[j]), (j, d[j], fa[j].dot(fb[j]))
        assert nn[j] == fa[j].squarednorm(), j
    al = np.array([0.5 - 0.25j * j for j in range(k)])
    A.axpy(al, B)
    for j in range(k):
        fa[j] = fa[j].add_scaled(al[j], fb[j])
        assert np.array_equal(A.column(j).to_numpy(), fa[j].to_numpy())
    assert not A.set_zero().to_numpy().any()


# ---- k-wide apply ---------------------------------------------------------------------------------------------------------
def check_apply(A, ncol, k):
    f = columns(ncol, k)
    Y = A.apply_multi(MultiField.from_fields(f)).to_numpy()
    for j in range(k):
        assert np.array_equal(Y[j], A(f[j]).to_numpy()), (k, j)


@pytest.mark.parametrize("n,patterns", [(16, True), (64, True), (128, True), (64, False)])
def test_apply_multi_poisson(n, patterns):
    A, N = poisson(n, patterns)
    if not patterns:
        assert A.storage_format()[0] == 0          # the plain ELL slab
    elif n >= 64:
        assert A.storage_format()[0] == 3          # the stencil view of the dictionary with values
    else:
        assert A.storage_format()[0] == 0          # below 2^15 rows no dictionary is tried
    for k in KS:
        check_apply(A, N, k)
    check_apply(DiracOp(A, 0.1 + 0.05j), N, 8)


def test_apply_multi_dictionary_forms():
    """both row-pattern dictionary forms through the generic kernel: form 1 without its stencil view, form 2 (a dictionary of
    the columns only: the values differ from row to row)"""
    prev = set_option("stencil_storage", 0)
    try:
        A, N = poisson(64)
        assert A.storage_format()[0] == 1
        for k in KS:
            check_apply(A, N, k)
        check_apply(DiracOp(A, 0.1 + 0.05j), N, 5)
    finally:
        set_option("stencil_storage", prev)
    n = 40
    N = n ** 3
    _, _, rowptr, col, val = problems.poisson3d_csr(n)
    val = val * (1.0 + np.random.default_rng(3).uniform(0, 1, val.size))
    B = Sparse(N, N, rowptr, col, val)
    assert B.storage_format()[0] == 2
    for k in KS:
        check_apply(B, N, k)
    check_apply(DiracOp(B, 0.1 + 0.05j), N, 5)


IRREGULAR = [   # the parameter sets of tests/test_gpu_bitwise.py::test_irregular_spmv_bit_for_bit; what each must exercise
    (257, 300, dict(min_len=0, max_len=9), ""),
    (3000, 2500, dict(min_len=0, max_len=6, long_rows=5, long_len=900), "tail"),
    (6000, 6000, dict(min_len=1, max_len=7, long_rows=7, long_len=3000), "tail"),
    (40000, 40000, dict(min_len=3, max_len=40), "tail"),
    (700, 700, dict(min_len=30, max_len=45), "lanes"),
    (64, 4096, dict(min_len=1000, max_len=1500), ""),
]


@pytest.mark.parametrize("nrow,ncol,kw,must", IRREGULAR)
def test_apply_multi_irregular(nrow, ncol, kw, must):
    rng = np.random.default_rng(nrow * 7 + ncol)
    A = Sparse(nrow, ncol, *problems.random_csr(nrow, ncol, rng, **kw))
    lay = A.ell_layout()
    if must == "tail":
        assert lay["tail_rows"] > 0, lay
    if must == "lanes":
        assert lay["lanes"] > 1, lay
    for k in KS:
        check_apply(A, ncol, k)
    if nrow == ncol:
        check_apply(DiracOp(A, 0.3 - 0.2j), ncol, 5)
        check_apply(DiracOp(A, 0.3 - 0.2j), ncol, 8)


def test_apply_multi_window_variant():
    N = 1 << 18
    A = Sparse(N, N, *problems.skewed_csr(N, np.random.default_rng(11), window=900, long_rows=3, long_len=2500))
    assert A.ell_layout()["x_window"] > 0
    for k in KS:
        check_apply(A, N, k)
    check_apply(DiracOp(A, 0.2 + 0.1j), N, 8)


def test_apply_multi_dirac_on_sample(sample):
    lay = sample.ell_layout()
    assert lay["lanes"] == 8, lay
    D = DiracOp(sample, 0.15 + 0.05j)
    for k in KS:
        check_apply(sample, sample.get_dim(), k)
        check_apply(D, sample.get_dim(), k)


@pytest.mark.parametrize("bs", [4, 20, 48])
def test_apply_multi_block_csr(bs):
    rng = np.random.default_rng(bs)
    nb = 300
    nt = 8 * nb
    rows = rng.integers(0, nb, nt).astype(np.int32)
    cols = rng.integers(0, nb, nt).astype(np.int32)
    rows[:40], cols[:40] = rows[40:80], cols[40:80]            # duplicate (row, col) pairs: kept, summed at apply time
    blocks = rng.uniform(-1, 1, (nt, bs, bs)) + 1j * rng.uniform(-1, 1, (nt, bs, bs))
    H = HierarchicalSparse(nb, nb, rows, cols, blocks)
    for k in KS:
        check_apply(H, nb * bs, k)


def test_apply_multi_dense():
    rng = np.random.default_rng(1)
    for dim in (7, 60):
        M = Dense(rng.uniform(-1, 1, (dim, dim)) + 1j * rng.uniform(-1, 1, (dim, dim)))
        for k in KS:
            check_apply(M, dim, k)


# ---- batched GCR ----------------------------------------------------------------------------------------------------------
def check_solve(A, n, param_args, k, rhs_cols=None, x0=None, use_x0=False):
    if isinstance(A, (Sparse, DiracOp)):
        assert A.xr_fuse_kind() in (0, 1)      # the premise of the bit-for-bit rule (include/mgcr.h)
    rhs = rhs_cols if rhs_cols is not None else columns(n, k, 1)
    prm = GCR_Param(*param_args, False, use_x0=use_x0)
    g = GCR(A, prm)
    X = MultiField.from_fields(x0) if x0 is not None else MultiField((n,), k).set_zero()
    g.solve_multi(MultiField.from_fields(rhs), X)
    its, conv, hist = g.last_iterations, g.last_converged, g.last_history
    Xh = X.to_numpy()
    for j in range(k):
        x = x0[j].copy() if x0 is not None else Field((n,)).set_zero()
        gs = GCR(A, prm)
        gs.solve(rhs[j], x)
        assert its[j] == gs.last_iterations, (j, its, gs.last_iterations)
        assert conv[j] == gs.last_converged, j
        assert np.array_equal(hist[j], gs.last_history), j
        assert np.array_equal(Xh[j], x.to_numpy()), j
    return its


@pytest.mark.parametrize("n", [32, 128])
@pytest.mark.parametrize("args", [(0, 5, 40, 0.0), (0, 3, 200, 1e-8)])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_solve_multi_poisson(n, args, k):
    A, N = poisson(n)
    check_solve(A, N, args, k)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_solve_multi_dirac_sample(sample, k):
    check_solve(DiracOp(sample, 0.15), sample.get_dim(), (0, 5, 300, 1e-13), k)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_solve_multi_block_csr(k):
    nb, bs = 600, 20
    H = HierarchicalSparse(nb, nb, *problems.unstructured_blocks(nb, bs))
    check_solve(H, nb * bs, (0, 5, 200, 1e-10), k)


@pytest.mark.parametrize("use_x0", [False, True])
def test_solve_multi_freezes_converged_columns(use_x0):
    n = 32
    A, N = poisson(n)
    s = np.sin(np.pi * np.arange(1, n + 1) / (n + 1))
    v = (s[:, None, None] * s[None, :, None] * s[None, None, :]).reshape(-1).astype(np.complex128)   # an exact eigenvector
    b1 = problems.rhs_grid(N, 1)
    cols = [Field((N,), v), Field((N,), b1), Field((N,), v * (np.linalg.norm(b1) / np.linalg.norm(v)) + b1)]
    x0 = [Field((N,), 0.01 * problems.rhs_grid(N, 7 + j)) for j in range(3)] if use_x0 else None
    its = check_solve(A, N, (0, 5, 400, 1e-4), 3, rhs_cols=cols, x0=x0, use_x0=use_x0)
    assert len(set(its)) == 3 and max(its) < 400, its     # three different stopping steps: the early columns were frozen


def test_solve_multi_small_system_takes_the_general_path():
    lib = _lib.lib()
    A, N = poisson(8)            # 512 rows: the single solve would run as one workgroup, in another summation order
    # (the library has no getter: the value in force is the environment's or the default, csrc/gcr_small.hip)
    old = int(os.environ.get("MGCR_SMALL_SOLVE_ROWS", "1024"))
    lib.mgcr_set_small_solve_rows(0)
    try:
        check_solve(A, N, (0, 5, 60, 1e-10), 4)
    finally:
        lib.mgcr_set_small_solve_rows(old)


# ---- errors, counters -----------------------------------------------------------------------------------------------------
def test_errors_and_counter():
    A, N = poisson(16)
    for k in (0, 17):
        with pytest.raises(MgcrError) as e:
            MultiField((N,), k)
        assert e.value.code == 1
    X = MultiField.from_fields(columns(N, 3))
    ref = X.to_numpy()

    def code(fn):
        with pytest.raises(MgcrError) as e:
            fn()
        return e.value.code

    assert code(lambda: A.apply_multi(X, out=X)) == 1
    assert code(lambda: A.apply_multi(X, out=MultiField((N,), 2))) == 1
    assert code(lambda: A.apply_multi(X, out=MultiField((N + 1,), 3))) == 1
    assert code(lambda: A.apply_multi(MultiField((N + 1,), 3), out=X)) == 1
    B = MultiField.from_fields(columns(N, 3, 5))
    assert code(lambda: GCR(A, GCR_Param(4, 0, 10, 1e-8, False)).solve_multi(B, X)) == 7           # truncation mode
    assert code(lambda: GCR(A, GCR_Param(0, 0, 10, 1e-8, False)).solve_multi(B, X)) == 7           # full mode
    inner = GCR(A, GCR_Param(0, 5, 2, 1e-8, False))
    assert code(lambda: GCR(A, GCR_Param(0, 5, 10, 1e-8, False, solver_r=inner, flexible=True)).solve_multi(B, X)) == 7
    assert code(lambda: GCR(A, GCR_Param(0, 5, 10, 1e-8, False, solver_l=inner)).solve_multi(B, X)) == 7
    assert code(lambda: GCR(A, GCR_Param(0, 5, 10, 1e-8, False)).solve_multi(B, MultiField((N,), 2))) == 1
    assert code(lambda: GCR(A, GCR_Param(0, 5, 10, 1e-8, False)).solve_multi(X, X)) == 1
    assert code(lambda: inner.apply_multi(B, out=X)) == 7                                          # a GCR object as operator
    assert np.array_equal(X.to_numpy(), ref)                                                       # X untouched by all of these
    before = stat("multi_solves")
    GCR(A, GCR_Param(0, 5, 10, 1e-8, False)).solve_multi(B, X)
    assert stat("multi_solves") == before + 1
