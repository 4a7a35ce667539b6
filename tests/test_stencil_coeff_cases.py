"""The premises of tests/stencil_coeff_cases.py, checked on the CPU with the oracle (no GPU):

  builder      box_csr has problems.poisson3d_box_csr's layout, every coefficient in exactly the rows whose neighbour is in range
  power        each of the 15 slot swaps moves the restart-5 history at step 1 by more than the loosest tolerance any test grants
               (tests/test_gpu_parity.py hist_close) — a kernel that mixes two slots up cannot pass even that
  control      the same swaps on Poisson's values move nothing: the blind spot of every test on the Poisson box, pinned
  convergence  GCR converges on both sets in restart, truncated and full mode
  table        the GPU cases' shapes are where their kernels run (row counts, oracle.row_map premises)
"""
import numpy as np
import pytest

from mgpreconditionedgcr_amd import problems
from oracle import oracle as orc
from tests import stencil_coeff_cases as sc

POWER_DIMS = (12, 10, 9)
BOXES = [(2, 2, 2), (3, 4, 5), (5, 3, 2), (4, 7, 3)]


def _reference_entries(nz, ny, nx, cs):
    """{(row, col): value} by the plainest loop there is"""
    out = {}
    steps = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))
    for i in range(nz):
        for j in range(ny):
            for k in range(nx):
                r = (i * ny + j) * nx + k
                out[(r, r)] = complex(cs.diag)
                for s, (di, dj, dk) in enumerate(steps):
                    ii, jj, kk = i + di, j + dj, k + dk
                    if 0 <= ii < nz and 0 <= jj < ny and 0 <= kk < nx:
                        out[(r, (ii * ny + jj) * nx + kk)] = complex(cs.off[s])
    return out


@pytest.mark.parametrize("which", ["real", "complex"])
def test_coefficient_sets_are_distinct_dyadic_and_not_symmetric(which):
    cs = sc.coeff_set(which)
    allv = np.array(cs.off + (cs.diag,), np.complex128)
    assert len(cs.off) == sc.SLOTS == 6 and len(sc.SWAPS) == 15
    assert np.array_equal(allv * 8, np.round(allv.real * 8) + 1j * np.round(allv.imag * 8))      # multiples of 1/8
    assert len(set(allv.real)) == 7                              # the diagonal included
    assert len(set(allv.imag[:6])) == (6 if which == "complex" else 1)     # the six off-diagonals (what a swap exchanges)
    for s in range(3):          # slot s couples r to r - o, slot 5 - s couples r - o back to r: different values, A != A^T
        assert cs.off[s] != cs.off[5 - s] and cs.off[s] != np.conj(cs.off[5 - s])
    for a, b in sc.SWAPS:
        m = sc.swapped(which, a, b)
        assert m.diag == cs.diag and m.off[a] == cs.off[b] and m.off[b] == cs.off[a]
        assert [s for s in range(6) if m.off[s] != cs.off[s]] == [a, b]


@pytest.mark.parametrize("which", ["real", "complex"])
@pytest.mark.parametrize("dims", BOXES)
def test_builder(dims, which):
    nz, ny, nx = dims
    cs = sc.coeff_set(which)
    N, ncol, rowptr, col, val = sc.box_csr(nz, ny, nx, which)
    assert N == ncol == nz * ny * nx and rowptr.dtype == np.int64 and col.dtype == np.int64 and val.dtype == np.complex128
    lens = np.diff(rowptr)
    assert rowptr[0] == 0 and rowptr[-1] == col.size == val.size and lens.min() >= 4 and lens.max() <= 7
    assert lens.min() == 4 and (lens.max() == 7) == (min(dims) >= 3)
    rows = np.repeat(np.arange(N), lens)
    inside = np.ones(col.size, bool)
    inside[rowptr[:-1]] = False
    assert (np.diff(col)[inside[1:]] > 0).all()                    # columns ascend within every row
    assert dict(zip(zip(rows.tolist(), col.tolist()), val.tolist())) == _reference_entries(nz, ny, nx, cs)
    # every coefficient in exactly the rows whose neighbour is in range (the values are pairwise distinct: a value names its slot)
    i, j, k = np.unravel_index(np.arange(N), dims)
    present = [i > 0, j > 0, k > 0, k < nx - 1, j < ny - 1, i < nz - 1]
    offset = [-ny * nx, -nx, -1, 1, nx, ny * nx]
    for s in range(6):
        at = val == cs.off[s]
        assert np.array_equal(np.sort(rows[at]), np.flatnonzero(present[s])) and (col[at] - rows[at] == offset[s]).all()
    assert np.array_equal(rows[val == cs.diag], np.arange(N)) and (col[val == cs.diag] == np.arange(N)).all()


@pytest.mark.parametrize("dims", BOXES + [POWER_DIMS, (6, 16, 32)])
def test_builder_reproduces_the_poisson_box(dims):
    ours, theirs = sc.box_csr(*dims, sc.POISSON), problems.poisson3d_box_csr(*dims)
    assert ours[:2] == theirs[:2]
    for a, b in zip(ours[2:], theirs[2:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert ours[4].tobytes() == theirs[4].tobytes()


def _history(which, **kw):
    N, ncol, rowptr, col, val = sc.box_csr(*POWER_DIMS, which)
    return orc.gcr_solve(orc.csr(N, ncol, rowptr, col, val), orc.gcr_param(max_iter=12, tol=sc.TOL, **kw), problems.rhs_grid(N, sc.RHS_SEED))[1]


@pytest.fixture(scope="module")
def unswapped():
    """name -> (restart-5 history, its re-association sensitivity), computed once"""
    out = {}
    for which in ("real", "complex"):
        N, ncol, rowptr, col, val = sc.box_csr(*POWER_DIMS, which)
        h, s, _ = orc.gcr_reorder_sensitivity(orc.csr(N, ncol, rowptr, col, val), orc.gcr_param(restart=5, max_iter=12, tol=sc.TOL),
                                              problems.rhs_grid(N, sc.RHS_SEED))
        h.setflags(write=False)
        out[which] = (h, s)
    return out


@pytest.mark.parametrize("which", ["real", "complex"])
def test_every_swap_moves_step_1_beyond_the_loosest_tolerance(unswapped, which):
    """(the oracle in index order, 12 x 10 x 9: the smallest move is 3.4e-5 of h(1) = 0.373 on the real set, swap (0, 5), and 5.6e-5 of
    0.409 on the complex one, swap (0, 3) — five orders of magnitude above the 4e-10 granted there)"""
    h, s = unswapped[which]
    granted =max(1e-9 * h[1], 8 * s[1]) + 1e-17          # tests/test_gpu_parity.py hist_close at step 1
    moved = {}
    for a, b in sc.SWAPS:
        hm = _history(sc.swapped(which, a, b), restart=5)
        moved[(a, b)] = abs(hm[1] - h[1])
    print(which, "h(1) = %.6e, granted %.3e, smallest move %.3e (relative %.3e) by swap %s"
          % (h[1], granted, min(moved.values()), min(moved.values()) / h[1], min(moved, key=moved.get)))
    assert all(m > granted for m in moved.values()), {k: m for k, m in moved.items() if m <= granted}


def test_swaps_on_poisson_values_move_nothing():
    """the blind spot: with six equal off-diagonals a slot mix-up gives the same matrix, hence the same bits"""
    h = _history(sc.POISSON, restart=5)
    ref = problems.poisson3d_box_csr(*POWER_DIMS)
    for a, b in sc.SWAPS:
        m = sc.swapped(sc.POISSON, a, b)
        assert np.array_equal(sc.box_csr(*POWER_DIMS, m)[4], ref[4])
        assert np.array_equal(_history(m, restart=5), h)


@pytest.mark.parametrize("mode", [dict(restart=5), dict(truncation=6), dict()], ids=["restart5", "truncation6", "full"])
@pytest.mark.parametrize("which", ["real", "complex"])
def test_gcr_converges(which, mode):
    h = _history(which, **mode)
    assert h.size == 13 and np.isfinite(h).all() and h[12] < h[0]
    if "restart" in mode:
        assert (np.diff(h) < 0).all()                       # monotonically


def test_case_table():
    cases = sc.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        N = int(np.prod(c.dims))
        assert N >= 1 << 15, c.id                              # below 2^15 rows no dictionary and no stencil view is tried
        assert len({v.id for v in c.variants}) == len(c.variants) and set(c.sets) <= set(sc.COEFFS)
        assert all((s.restart == 0 or s.truncation == 0) and s.max_iter >= 1 for s in c.solves)
        for v in c.variants:
            assert set(v.dirac) <= set(c.solves) and all(rel in (">0", "==0", "==1", "print") for _, rel in v.counters + v.dirac_counters)
        if c.group == "steps":                                 # the one-launch steps' range: 512 logical workgroups, <= 4 rows per thread
            assert 2 ** 19 < N <= 2 ** 21 and all(0 < s.restart <= 5 for s in c.solves), c.id
        if c.group in ("resident", "fused"):
            assert N < 64 * 1024, c.id                         # fewer than 64 workgroups of 1024 rows
        if c.premise:
            assert sc.row_map_premise(c.premise, c.dims, orc.row_map, orc.row_map_plane), c.id
        elif c.group == "window":
            assert orc.row_map_plane(N, c.dims[1] * c.dims[2]) == 0
    assert {c.group for c in cases} == {"resident", "fused", "steps", "carry", "window"}
    assert (sc.KIND2_NZ, 256, 256) in [c.dims for c in cases]
    for dims, which in sc.DIST_KINDS.values():
        assert which in sc.COEFFS and int(np.prod(dims)) // 3 >= 1 << 15      # a stencil view on each of three ranks
