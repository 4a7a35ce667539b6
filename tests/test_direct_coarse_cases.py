"""CPU check of the direct coarsest solve's case table and reference model (tests/direct_coarse_cases.py): the premises
tests/test_gpu_direct_coarse.py relies on.  No case is skipped: a case whose premise fails is a failing test."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import direct_coarse_cases as dc

BOUND = dc.BOUND_CASES
ids = lambda cases: [c.id for c in cases]     # noqa: E731


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_table_covers_what_it_must():
    assert len(set(ids(dc.all_cases()))) == len(dc.all_cases())
    piv = {(c.n, c.cplx) for c in BOUND if c.kind == "pivot"}
    assert {n for n, _ in piv} == {1, 2, 3, 5, 63, 64, 65, 255, 257, 1023, 1024, 1025, 1500, 2048}
    assert {(65, False), (65, True), (257, False), (257, True)} <= piv
    assert [(c.n, c.k.imag != 0) for c in BOUND if c.kind == "dirac"] == [(257, True)]
    assert [c.n for c in BOUND if c.kind == "tie"] == [130] and [c.kind for c in BOUND].count("general") == 1
    assert {(c.n, c.direct) for c in dc.KEPT_CASES} == {(2049, 4096), (257, 256)}
    assert 2049 % 2 == 1      # odd (3 x 683): no two-row aggregates to fall back to
    assert [c.kind for c in dc.SINGULAR_CASES] == ["zero_column", "equal_rows", "zero_1x1"]
    assert {(c.n, c.ea, c.eb) for c in dc.SCALED_AS_STATED} == {(65, -600, -600), (65, 600, 600)}
    for c in dc.SCALED_AS_STATED + dc.SCALED_IN_RANGE:      # the n = 65 case, times a power of two
        base = dc.problem(next(b for b in BOUND if b.id == "pivot-65-complex"))
        assert np.array_equal(dc.problem(c).A, np.ldexp(base.A.real, c.ea) + 1j * np.ldexp(base.A.imag, c.ea))
    assert dc.HEALTHY.id == "pivot-64"
    assert dc.K == 2.0 ** round(np.log2(dc.K))


@pytest.mark.parametrize("case", [c for c in dc.all_cases() if c.kind != "general"], ids=ids([c for c in dc.all_cases() if c.kind != "general"]))
def test_one_row_aggregates_make_the_coarse_operator_the_fine_one(case):
    """mesh (n,), subblock 1, one vector of ones: prolongator all ones, agg the identity, level-1 operator = the fine operator bit for bit
    (all unit vectors up to 257 rows, 16 of them above — what the GPU test asserts of the device)"""
    p = dc.problem(case)
    Mo = dc.oracle_mg(case, p, orc.gcr_param(**dc.SLOPPY))
    pv, agg = Mo.prolongator(0)
    assert np.array_equal(pv, np.ones((p.N, 1))) and np.array_equal(agg, np.arange(p.N))
    Ac, Af = Mo.level_op(1), orc.dirac(orc.csr(p.N, p.N, p.rowptr, p.col, p.val), p.shift) if p.shift is not None else None
    for j in dc.unit_columns(p.N):
        e = np.zeros(p.N, np.complex128)
        e[j] = 1.0
        col = Ac(e)
        if Af is None:
            assert np.array_equal(col, p.A[:, j]), j
        else:       # under a shift the host's Id - k D is rounded once more than x - k (D x): the oracle's own fine operator is the twin
            assert np.array_equal(col, Af(e)) and np.abs(col - p.A[:, j]).max() <= 4 * dc.U * np.abs(p.A[:, j]).max(), j


def test_prolongator_matrix_is_the_oracles_restrict_and_expand():
    case = next(c for c in BOUND if c.kind == "general")
    p = dc.problem(case)
    Mo = dc.oracle_mg(case, p, orc.gcr_param(**dc.SLOPPY))
    pv, agg = Mo.prolongator(0)
    P = dc.prolongator_matrix(pv, agg)
    assert P.shape == (128, 64) and np.abs(P.conj().T @ P - np.eye(64)).max() <= 1e-14
    x, xc = dc.problem(case).b, np.random.default_rng(0).standard_normal(64) + 0.5j
    assert np.abs(P.conj().T @ x - orc.mg_restrict(agg, 32, pv, x)).max() <= 1e-14
    assert np.abs(P @ xc - orc.mg_expand(agg, pv, xc)).max() <= 1e-14


@pytest.mark.parametrize("case", BOUND, ids=ids(BOUND))
def test_the_model_is_the_projects_cycle(case):
    """on the case's matrix with a dominant diagonal the oracle's coarsest GCR converges: `model` must then be the oracle's cycle with
    damping 0.5 to 10 times the relative residual that GCR reached (or one unit roundoff, where it reached less: the model and the oracle
    round differently)"""
    p = dc.problem(case, 16.0)
    coarse = orc.gcr_param(restart=0, max_iter=400, tol=1e-13)
    Mo = dc.oracle_mg(case, p, coarse)
    P, Ac = dc.host_hierarchy(case, 16.0)
    yo = Mo(p.b)
    seen = {}

    def solve(bc):
        seen["bc"] = bc
        return np.linalg.solve(Ac, bc)

    ym = dc.model(p.A, p.b, P, solve)
    _, hist, it, conv = orc.gcr_solve(Mo.level_op(1), coarse, seen["bc"])
    assert conv and it < 400 and hist[-1] <= 1e-13
    reached = max(hist[-1], dc.U)
    dev = np.abs(ym - yo).max() / np.abs(yo).max()
    assert dev <= 10 * reached, (dev, reached)
    # ... and the cycle without the damping is not (one row: every cycle solves the system)
    if p.N == 1:
        return
    wrong = dc.model(p.A, p.b, P, solve, damping=1.0)
    assert np.abs(wrong - yo).max() / np.abs(yo).max() > 1e4 * reached


@pytest.mark.parametrize("case", BOUND + dc.SCALED_IN_RANGE, ids=ids(BOUND + dc.SCALED_IN_RANGE))
def test_conditioning_refinement_and_pivoting(case):
    ref = dc.host_reference(case)
    nc = dc.host_hierarchy(case)[1].shape[0]
    assert np.isfinite(ref.y.astype(np.complex128)).all() and np.isfinite(ref.e_ref)
    assert ref.kappa <= 1e6
    assert ref.residual <= 1e-17 * ref.bnorm, (ref.residual, ref.bnorm)
    assert ref.e_ref <= 64 * nc * dc.U * ref.kappa        # the reference's own error is of the size the bound's floor speaks of
    el = dc.host_elimination(case)
    assert el is not None
    if nc >= 2:                                           # (one row has nothing to swap with)
        assert 2 * el.swaps >= nc, (el.swaps, nc)
    if nc > dc.PIVOT_THREADS:
        assert el.far >= 1
    assert np.abs(el.inv @ dc.host_hierarchy(case)[1] - np.eye(nc)).max() <= 1e-11     # the host elimination inverts


@pytest.mark.parametrize("n", [255, 257])
def test_blocked_elimination_finds_the_unblocked_pivots(n):
    case = next(c for c in BOUND if c.n == n and c.kind == "pivot")
    Ac = dc.host_hierarchy(case)[1]
    a, b = dc.gauss_jordan(Ac), dc.blocked_pivots(Ac, nb=32)
    assert np.array_equal(a.pivots, b.pivots) and np.abs(a.inv - b.inv).max() <= 1e-13


def test_the_tie_is_a_tie():
    case = next(c for c in BOUND if c.kind == "tie")
    Ac = dc.host_hierarchy(case)[1]
    a = dc.rank_squares(Ac[:, 0])
    lo, hi = dc.TIE_ROWS
    assert a[lo] == a[hi] == 25.0 and np.delete(a, [lo, hi]).max() < 1.0
    assert lo < 64 <= hi < 128 and hi - lo == 64          # step 0: threads lo and hi, merged at stride 64 of the tree
    assert dc.gauss_jordan(Ac).pivots[0] == lo


def mutant_fails(case, el):
    """a mutant's elimination fails on a case: "singular", or the model with its inverse misses the bound by a factor of 1000 or more"""
    if el is None:
        return True
    p, ref = dc.problem(case), dc.host_reference(case)
    P, _ = dc.host_hierarchy(case)
    y = dc.model(p.A, p.b, P, lambda bc: el.inv @ bc)
    return not np.isfinite(y).all() or dc.error_of(y, ref) >= 1000 * dc.bound_of(ref)


def test_the_cases_discriminate_a_search_that_stops_after_1024_candidates():
    """(below 1024 rows the window never binds: the mutant is the elimination itself)"""
    big = [c for c in BOUND if c.n > dc.PIVOT_THREADS]
    assert len(big) == 3
    failed = [c.id for c in big if mutant_fails(c, dc.blocked_pivots(dc.host_hierarchy(c)[1], window=dc.PIVOT_THREADS))]
    assert "pivot-1500" in failed, failed
    assert not any(mutant_fails(c, dc.host_elimination(c)) for c in big)       # the elimination itself does not


def test_the_cases_discriminate_an_identity_half_that_is_not_swapped():
    """(the unblocked elimination: the cases up to 257 rows)"""
    small = [c for c in BOUND if dc.host_hierarchy(c)[1].shape[0] <= dc.FAITHFUL_MAX_ROWS]
    failed = [c.id for c in small if mutant_fails(c, dc.gauss_jordan(dc.host_hierarchy(c)[1], swap_identity=False))]
    assert len(failed) >= len(small) - 1, failed                               # every case that swaps at all (pivot-1 cannot)
    assert not any(mutant_fails(c, dc.host_elimination(c)) for c in small)


@pytest.mark.parametrize("case", dc.SINGULAR_CASES, ids=ids(dc.SINGULAR_CASES))
def test_singular_cases_are_singular_to_the_elimination(case):
    A = dc.problem(case).A
    assert dc.gauss_jordan(A) is None and dc.gauss_jordan(A, rank=dc.rank_squares) is None
    if case.kind == "equal_rows":
        assert np.array_equal(A[0], A[2]) and np.array_equal(A, A.real.round())


@pytest.mark.parametrize("case", [c for c in BOUND if c.n <= dc.FAITHFUL_MAX_ROWS], ids=ids([c for c in BOUND if c.n <= dc.FAITHFUL_MAX_ROWS]))
def test_scaled_ranking_keeps_the_pivots_of_the_normal_range(case):
    """ranking by the column scaled by a power of two = ranking by x^2 + y^2 wherever that neither overflows nor underflows: the same
    pivots and the same bits"""
    Ac = dc.host_hierarchy(case)[1]
    a, b = dc.gauss_jordan(Ac, rank=dc.rank_squares), dc.gauss_jordan(Ac, rank=dc.rank_scaled)
    assert np.array_equal(a.pivots, b.pivots) and np.array_equal(a.inv, b.inv)


def test_what_squares_do_to_a_scaled_matrix():
    """x^2 + y^2 underflows to zero for every entry of 2^-600 A (a regular matrix ends "singular") and overflows to infinity for every
    entry of 2^+600 A (the search degrades to "the first nonzero row"); the scaled modulus keeps the pivots of A"""
    base = dc.gauss_jordan(dc.problem(next(b for b in BOUND if b.id == "pivot-65-complex")).A)
    down, up = (dc.problem(c).A for c in dc.SCALED_IN_RANGE)
    assert dc.gauss_jordan(down, rank=dc.rank_squares) is None
    first = dc.gauss_jordan(up, rank=dc.rank_squares)
    assert first is not None and not np.array_equal(first.pivots, base.pivots)
    for A, e in ((down, 600), (up, -600)):
        el = dc.gauss_jordan(A)
        assert np.array_equal(el.pivots, base.pivots)
        assert np.array_equal(np.ldexp(el.inv.real, -e) + 1j * np.ldexp(el.inv.imag, -e), base.inv)


@pytest.mark.parametrize("case", dc.SCALED_AS_STATED, ids=ids(dc.SCALED_AS_STATED))
def test_the_smoother_leaves_the_number_range_when_b_is_scaled_like_the_matrix(case):
    """why tests/test_gpu_direct_coarse.py marks these two xfail: with A and b both times 2^-+600 the one-step smoother's <Ap, Ap> is of
    size 2^-+2400 — the cycle in complex128 is not finite whatever the coarsest solve does, and only the extended-precision truth is"""
    p = dc.problem(case)
    with np.errstate(all="ignore"):
        ref = dc.host_reference(case)
        r = p.b
        Ap = p.A @ r
        den = np.vdot(Ap, Ap)
    assert den == 0 or not np.isfinite(den)
    assert not np.isfinite(ref.e_ref) and np.isfinite(ref.y.astype(np.clongdouble)).all()
