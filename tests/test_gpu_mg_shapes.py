"""The device's multigrid set-up and transfer kernels off the 2^d aggregate path, against the oracle (tests/mg_shape_cases.py holds
the cases, tests/test_mg_shape_cases.py their premises and the oracle's own pinning: an independent extended-precision model, and the
real reference's golden at block edge 4).

Per case, as tests/test_gpu_mg_fuzz.py does at edge 2: aggregate map, prolongator and every entry of every coarse operator (dense view)
bit for bit, restrict bit for bit, expand to 1e-15 and one V-cycle (2 sweeps of GCR(10), coarsest GCR(10) of 40 steps to 1e-3) to 1e-9 of
their largest entry; the projector identities R P R = R and P R P R = P R to 1e-13 and R A P w = A_c w to 1e-12.  Premises only the
device can show — the CSR tail, the offsets-only dictionary, the block-CSR operator, the uniform-prolongator shortcut — are asserted
on the device objects before anything is compared.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

mg = pytest.importorskip("mgpreconditionedgcr_amd")
from mgpreconditionedgcr_amd import DiracOp, Field, GCR, GCR_Param, HierarchicalSparse, MG, MG_Param, Mesh, Sparse, problems  # noqa: E402
from tests import mg_shape_cases as ms  # noqa: E402

CASES, IDS = ms.CASES, ms.IDS


@pytest.fixture(scope="module", autouse=True)
def _init():
    mg.init()
    yield


def device_operator(case):
    """(A, base): the case's fine operator on the device (a Sparse, a HierarchicalSparse, or a DiracOp around one) and its matrix"""
    p = ms.problem(case)
    if p.triplets is not None:
        nb, bs, rows, cols, blocks = p.triplets
        base = HierarchicalSparse(nb, nb, rows, cols, blocks)
    else:
        base = Sparse(p.N, p.N, p.rowptr, p.col, p.val)
    return (DiracOp(base, p.shift) if p.shift is not None else base), base


def device_mg(case, A):
    p = ms.problem(case)
    prm = MG_Param(Mesh(case.dims), case.sub, case.ne, None, GCR(GCR_Param(0, 10, 40, 1e-3, False)), GCR(GCR_Param(0, 10, 2, 1e-30, False)),
                   case.levels, None, None, spacetime=[bool(b) for b in case.blocked], null_vectors=p.vecs)
    return MG(A, prm)


def coarse_dense(M, l):
    nc = M.level_info(l)["dim"]
    Ac = M.level_operator(l)
    return ms.dense_view(lambda e: Ac(Field((nc,), e)).to_numpy(), nc)


def storage_premise(case, base):
    """what the case's row of the table says about how the device stores the fine operator"""
    if case.id == "tail":          # Galerkin rows read from the CSR tail: for_each_entry's binary search in trows
        assert base.stored_bytes()["tail_nnz"] > 2000 and base.ell_layout()["tail_rows"] >= 5      # the five long rows' entries
    if case.id == "dict-offsets":  # pat_mode == 2: column offsets in the dictionary, values in the slab
        assert base.storage_format()[0] == 2 and base.stored_bytes()["tail_nnz"] == 0
    if case.id == "block-op":      # for_each_entry's block-CSR branch
        assert isinstance(base, HierarchicalSparse) and base.bs == 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hierarchy_vs_oracle(case):
    p = ms.problem(case)
    Mo = ms.oracle_mg(case)
    A, base = device_operator(case)
    storage_premise(case, base)
    M = device_mg(case, A)
    dims = case.dims
    for l in range(case.levels):
        pv, agg = M.prolongator(l)
        pvo, aggo = Mo.prolongator(l)
        assert M.level_info(l)["ne"] == case.ne
        assert np.array_equal(agg, aggo), l
        assert np.array_equal(pv, pvo), l
    for l in range(1, case.levels + 1):
        assert M.level_info(l)["dim"] == Mo.level_dim(l)
        assert np.array_equal(coarse_dense(M, l), ms.dense_view(Mo.level_op(l), Mo.level_dim(l))), l
    # the transfers of every level (level 0 on the case's mesh, the coarser ones on plain vectors)
    for l in range(case.levels):
        n = M.level_info(l)["dim"]
        v = problems.rhs_grid(n, 7 + l)
        Rv = M.restrict(Field(dims if l == 0 else (n,), v), level=l)
        Rvo = Mo.restrict(l, v)
        assert np.array_equal(Rv.to_numpy().ravel(), Rvo), l
        PRv = M.expand(Rv, level=l).to_numpy().ravel()
        assert np.abs(PRv - Mo.expand(l, Rvo)).max() <= 1e-15 * max(np.abs(PRv).max(), 1.0), l
    v = problems.rhs_grid(p.N, 7)
    y = M(Field(dims, v)).to_numpy().ravel()
    yo = Mo(v)
    assert np.abs(y - yo).max() <= 1e-9 * np.abs(yo).max()
    # projector identities: R P = 1 on the coarse space, hence R P R = R and P R P R = P R; Galerkin consistency R A P w = A_c w
    f = Field(dims).fill_rhs(3)
    Rf = M.restrict(f)
    PRf = M.expand(Rf)
    RPRf = M.restrict(PRf)
    assert (RPRf - Rf).norm() <= 1e-13 * Rf.norm()
    assert (M.expand(RPRf) - PRf).norm() <= 1e-13 * PRf.norm()
    w = Field((M.level_info(1)["dim"],)).fill_rhs(4)
    lhs = M.restrict(A(M.expand(w)))
    rhs_c = M.level_operator(1)(w)
    assert (lhs - rhs_c).norm() <= 1e-12 * rhs_c.norm()


@pytest.mark.parametrize("id", ms.UNIFORM_CASES)
def test_uniform_prolongator_shortcut_keeps_the_bits(id, monkeypatch):
    """MgLevel::pv_uniform (one constant vector over aggregates of one size: the transfer kernels do not read the prolongator) with
    27-member aggregates (partial batches, paired and unpaired full ones) and with 64-member ones over a dictionary operator: the
    hierarchy built with the shortcut and with MGCR_MG_UNIFORM_PV=0 (read at every create) restricts, expands and cycles to the same
    bits — and both are the oracle's (test_hierarchy_vs_oracle runs the default)."""
    case = ms.BY_ID[id]
    p = ms.problem(case)
    A, base = device_operator(case)
    storage_premise(case, base)
    pv0 = ms.oracle_mg(case).prolongator(0)[0]
    assert case.ne == 1 and (pv0 == pv0[0]).all()          # the prolongator IS uniform: the scan at set-up finds it so
    got = []
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("MGCR_MG_UNIFORM_PV", raising=False)
        else:
            monkeypatch.setenv("MGCR_MG_UNIFORM_PV", setting)
        M = device_mg(case, A)
        v = Field(case.dims, problems.rhs_grid(p.N, 7))
        Rv = M.restrict(v)
        got.append((Rv.to_numpy().ravel(), M.expand(Rv).to_numpy().ravel(), M(v).to_numpy().ravel()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0][0], ms.oracle_mg(case).restrict(0, problems.rhs_grid(p.N, 7)))


def test_sample_edge4_vs_reference():
    """The device directly against the real reference's golden at block edge 4 (tests/golden/mg_4x4_edge4.npz: one aggregate of all
    3072 unknowns, 4 vectors — one thread of gs_kernel / gal_fill_kernel works through 3072 members): prolongator columns and R v bit for
    bit, P R v, A_c R v and the dense A_c to test_g9_pieces_vs_reference's tolerances; then the MG-preconditioned flexible GCR(5)
    converges, its true residual equal to its recurrence residual."""
    g = ms.golden_edge4()
    case = ms.BY_ID["sample-edge4"]
    A, _ = device_operator(case)
    M = device_mg(case, A)
    assert M.level_info(0) == dict(dim=3072, ne=4, nagg=1) and M.level_info(1)["dim"] == 4
    pv, agg = M.prolongator(0)
    assert not agg.any()
    for k in range(4):
        assert np.array_equal(pv[:, k], g["P"][0, k]), k
    v = Field(case.dims, g["v"])
    Rv = M.restrict(v)
    assert np.array_equal(Rv.to_numpy(), g["Rv"])
    assert np.abs(M.expand(Rv).to_numpy().ravel() - g["PRv"]).max() <= 1e-15
    Ac = M.level_operator(1)
    assert np.abs(Ac(Rv).to_numpy() - g["AcRv"]).max() <= 1e-14 * np.abs(g["AcRv"]).max()
    assert np.abs(coarse_dense(M, 1) - g["Ac_dense"]).max() <= 1e-15 * np.abs(g["Ac_dense"]).max()
    rhs = Field(case.dims).fill_rhs(4)
    x = Field(case.dims).set_zero()
    outer = GCR(A, GCR_Param(0, 5, 200, 1e-8, False, None, M, flexible=True, check_every=1))
    outer.solve(rhs, x)
    assert outer.last_converged and outer.last_history[-1] <= 1e-8
    true_rel = (rhs - A(x)).norm() / rhs.norm()
    assert abs(true_rel - outer.last_history[-1]) <= 1e-6 * outer.last_history[-1]
