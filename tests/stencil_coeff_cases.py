"""Seven-point box operators with seven DISTINCT coefficients, and the table of GPU cases that run them through every stencil solve
path (a plain module, like tests/multi_rhs_cases.py — not a test file; host only, numpy).

Why: the Poisson box (problems.poisson3d_box_csr) has six equal off-diagonals.  A kernel that pairs the right x with the wrong slot's
coefficient, or the real part of one slot with the imaginary part of another, gives the same bits on it — so neither the comparison
with the oracle nor any "path A == path B" test can see such a mix-up.  The operators here are non-symmetric, their six off-diagonals
are pairwise distinct in the real and in the imaginary part, and every value is dyadic (a multiple of 1/8): products with the 0.001
grid of problems.rhs_grid round like any other, nothing cancels by accident.

tests/test_stencil_coeff_cases.py (CPU) checks the premises with the oracle: the builder, that every one of the 15 slot swaps moves the
residual history by more than the loosest tolerance any test grants, that the same swaps on Poisson's values move nothing, and that
GCR converges on both sets.  tests/test_gpu_stencil_coeffs.py runs the table below on the GPU; tests/dist_worker.py builds the kinds
"coeffs48" / "coeffs48c" from box_csr for tests/test_gpu_dist.py::test_distributed_stencil_coefficients.
"""
from collections import namedtuple

import numpy as np

# slot order: (-ny*nx, -nx, -1, +1, +nx, +ny*nx) — ascending column; the diagonal sits between slots 2 and 3
SLOTS = 6
CoeffSet = namedtuple("CoeffSet", "off diag")
COEFFS = {
    "real": CoeffSet((-1.75, -0.5, -1.25, -0.75, -1.5, -0.25), 6.5),
    "complex": CoeffSet((-1.75 + 0.25j, -0.5 - 0.75j, -1.25 + 0.5j, -0.75 - 0.25j, -1.5 + 0.125j, -0.25 + 1j), 7 + 0.5j),
}
POISSON = CoeffSet((-1.0,) * SLOTS, 6.0)       # problems.poisson3d_box_csr's values: the control
SWAPS = [(a, b) for a in range(SLOTS) for b in range(a + 1, SLOTS)]     # the 15 mutants


def coeff_set(which):
    """`which`: a name in COEFFS, or a CoeffSet (what `swapped` returns)"""
    return COEFFS[which] if isinstance(which, str) else CoeffSet(tuple(which[0]), which[1])


def swapped(which, a, b):
    """the coefficient set with the off-diagonal slots a and b exchanged"""
    c = coeff_set(which)
    off = list(c.off)
    off[a], off[b] = off[b], off[a]
    return CoeffSet(tuple(off), c.diag)


def box_csr(nz, ny, nx, which):
    """(N, ncol, rowptr, col, val) of the 7-point operator on an nz x ny x nx box in problems.poisson3d_box_csr's layout: rows
    r = (i*ny + j)*nx + k, an entry per in-range neighbour (truncated boundaries), columns ascending within a row."""
    c = coeff_set(which)
    i, j, k = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    r = (i * ny + j) * nx + k
    cand = [(i > 0, r - ny * nx, c.off[0]), (j > 0, r - nx, c.off[1]), (k > 0, r - 1, c.off[2]),
            (np.ones_like(r, bool), r, c.diag),
            (k < nx - 1, r + 1, c.off[3]), (j < ny - 1, r + nx, c.off[4]), (i < nz - 1, r + ny * nx, c.off[5])]
    mask = np.stack([m for m, _, _ in cand], axis=1)
    cols = np.stack([cc for _, cc, _ in cand], axis=1)
    vals = np.broadcast_to(np.array([v for _, _, v in cand], np.complex128), mask.shape)
    rowptr = np.zeros(r.size + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=rowptr[1:])
    return r.size, nz * ny * nx, rowptr, cols[mask], vals[mask].astype(np.complex128)


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------------
# Solve: GCR mode and length.  restart / truncation as in GCR_Param (both 0: full mode); the tolerance is never met.
Solve = namedtuple("Solve", "restart truncation max_iter")
TOL = 1e-30
RHS_SEED, X_SEED = 3, 5                 # problems.rhs_grid seeds: the solves' right-hand side, the applies' input
DIRAC_K = 0.11 - 0.07j                  # the DiracOp cases: 1 - k A


def R(restart, max_iter):
    return Solve(restart, 0, max_iter)


def T(truncation, max_iter):
    return Solve(0, truncation, max_iter)


def F(max_iter):
    return Solve(0, 0, max_iter)


# Variant: one run of a case's solves.
#   build     options in force while the Sparse is built   ((name, value), ...)
#   options   options in force during the solves
#   format    what Operator.storage_format() must report ((fmt, slots); slots None: not looked at)
#   counters  what the counter's increase over ONE solve must satisfy: (stat name, ">0" | "==0" | "==1" | "print")
#   dirac     the Solves that run a second time on DiracOp(A, DIRAC_K) (with its stand-alone apply); the counters then asserted are
#             `dirac_counters`
Variant = namedtuple("Variant", "id build options format counters dirac dirac_counters")
# Case: dims (nz, ny, nx); sets: the coefficient sets it runs with; premise: the row-map premise the GPU test asserts before it
# solves (None | "kind2-square" | "kind2-plane" | "kind2-ragged"), mirrored on the CPU in tests/test_stencil_coeff_cases.py
Case = namedtuple("Case", "id group dims sets solves variants premise")


def _variant(id, build=(), options=(), format=(3, 7), counters=(), dirac=(), dirac_counters=None):
    return Variant(id, tuple(build), tuple(options), format, tuple(counters), tuple(dirac), tuple(counters if dirac_counters is None else dirac_counters))


BOTH = ("real", "complex")
RESIDENT_DIMS = (33, 32, 34)            # 35 904 rows: above the dictionary's 2^15, inside the resident solver's range
STEP_DIMS = (96, 96, 57)                # 525 312 rows: the one-launch steps (512 logical workgroups)
STEP_DIMS_WIDE = (96, 120, 112)         # 1 290 240 rows: threads with 2 and with 3 rows

_NO_RES = (("resident_solver", 0),)
_ONE_RES, _NO_RES_RAN = (("resident_solves", "==1"),), (("resident_solves", "==0"),)


def _storages(**kw):
    """the stencil view (format 3, 7 slots) and the row-pattern dictionary with values (format 1), whose pattern-to-value lookup is
    as blind on Poisson as the stencil's slot table"""
    return (_variant("stencil", **kw), _variant("dictionary", build=(("stencil_storage", 0),), format=(1, None), **kw))


def _resident_cases():
    solves = (R(10, 23), R(5, 12))
    fused = (R(4, 11), R(10, 2), T(3, 9), F(9))     # restart cycles, the fused step 0, truncated and full GCR (the classic kernels)
    return [
        Case("resident", "resident", RESIDENT_DIMS, BOTH, solves, _storages(counters=_ONE_RES, dirac=(R(5, 12),)), None),
        Case("fused-multi-kernel", "fused", RESIDENT_DIMS, BOTH, fused, _storages(options=_NO_RES, counters=_NO_RES_RAN), None),
    ]


def _step_cases():
    late, pair, own, steps, start = "step_pair_late_launches", "step_pair_launches", "step_apply_own_launches", "step_build_launches", "start_build_launches"
    keep = ((steps, ">0"), (own, ">0"))
    # a DiracOp keeps the keep forms: a one-launch step whose apply takes the own r from the diagonal gather, no pair kernel
    shifted = keep + ((late, "==0"), (pair, "==0"))
    real = (
        _variant("default", counters=keep + ((late, ">0"), (pair, ">0"), (start, "==1")), dirac=(R(5, 12),), dirac_counters=shifted),
        _variant("late-2", options=(("step_build_pair_late", 2),), counters=keep + ((late, ">0"), (pair, ">0"))),
        _variant("late-0", options=(("step_build_pair_late", 0),), counters=keep + ((late, "==0"), (pair, ">0"))),
        _variant("pair-0", options=(("step_build_pair", 0),), counters=keep + ((late, "==0"), (pair, "==0"))),
        _variant("keep-all-0", options=(("step_build_keep_all", 0),), counters=((steps, ">0"), (own, "==0"), (late, "==0"), (pair, "==0"))),
        _variant("step-build-0", options=(("step_build", 0),), counters=((steps, "==0"), (own, "==0"), (late, "==0"), (pair, "==0"))),
        _variant("start-build-0", options=(("start_build", 0),), counters=keep + ((late, ">0"), (start, "==0"))),
    )
    # complex coefficients: the REALC = false kernels; which pair forms they get is printed, not asserted
    cplx = (
        _variant("default", counters=((steps, ">0"), (late, "print"), (pair, "print"), (own, "print"))),
        _variant("step-build-0", options=(("step_build", 0),), counters=((steps, "==0"),)),
    )
    settings = (R(5, 12), R(4, 9))
    return [
        Case("steps-real", "steps", STEP_DIMS, ("real",), settings, real, None),
        Case("steps-complex", "steps", STEP_DIMS, ("complex",), settings, cplx, None),
        Case("steps-wide-box", "steps", STEP_DIMS_WIDE, ("real",), (R(5, 12),), (real[0]._replace(dirac=()),), None),
    ]


KIND2_NZ = 8      # tests/multi_rhs_cases.py KIND2_NZ: 8 x 256 x 256 = 512 x 1024 rows, the smallest slab with a full grid
# Operator.xr_fuse_kind() on the carried-window shapes.  The carried far slots and the residual update inside the windowed apply are built
# for REAL stencil coefficients (csrc/gcr_fused.hip tile_carry: row_mat(...).realv): the real set takes them (kind 2, |r|^2 over the apply's
# row map).  The complex set runs the same row maps through the windowed kernels with the far slots GATHERED and the update kernel
# separate (kind 0) — the forms a real operator only takes with MGCR_TILE_CARRY=0 in a child process.
XR_FUSE_KIND = {"real": 2, "complex": 0}


def _carry_cases():
    v = (_variant("default"),)
    return [
        Case("carry-8x256x256", "carry", (KIND2_NZ, 256, 256), BOTH, (R(5, 7), R(3, 3), T(6, 10)), v, "kind2-square"),
        Case("carry-6x256x512", "carry", (6, 256, 512), BOTH, (R(5, 7), R(3, 3)), v, "kind2-plane"),
        Case("carry-24x200x200", "carry", (24, 200, 200), BOTH, (R(5, 7), R(3, 3)), v, "kind2-ragged"),
    ]


def _window_cases():
    v = (_variant("default"),)
    solves = (R(4, 11), R(10, 2))          # restart cycles; a smoother-shaped solve (the fused step 0)
    return [
        Case("window-4x300x300", "window", (4, 300, 300), BOTH, solves, v, None),      # the 1024-row LDS window
        Case("window-5x200x200", "window", (5, 200, 200), BOTH, solves, v, None),      # the 512-row window
    ]


def all_cases():
    return _resident_cases() + _step_cases() + _carry_cases() + _window_cases()


def case_params():
    """(case, coefficient set name) pairs, with ids"""
    return [(c, w) for c in all_cases() for w in c.sets]


# the k-wide apply and the batched solve
MULTI_APPLY_DIMS = (RESIDENT_DIMS, STEP_DIMS)
MULTI_APPLY_KS = (1, 5, 8)
MULTI_SOLVE_DIMS, MULTI_SOLVE_K, MULTI_SOLVE = RESIDENT_DIMS, 3, R(5, 7)

# the distributed kinds of tests/dist_worker.py: name -> (dims, coefficient set); granularity one plane
DIST_KINDS = {"coeffs48": ((48, 48, 48), "real"), "coeffs48c": ((48, 48, 48), "complex")}


def row_map_premise(premise, dims, row_map, row_map_plane):
    """the premise of a carried-window case as the existing tests of these shapes assert it (tests/test_gpu_bitwise.py), from
    oracle.row_map / row_map_plane — `reach` of a box operator is its plane"""
    nz, ny, nx = dims
    N, plane = nz * ny * nx, ny * nx
    band, per = row_map(N, plane)
    if premise == "kind2-square":          # test_poisson_256x256_slab_carried_window_bit_for_bit
        return band > 0 and per * 1024 == plane
    if premise == "kind2-plane":           # test_plane_walk_row_map_on_boxes_bit_for_bit
        return band > 0 and per == plane // 1024
    if premise == "kind2-ragged":          # test_ragged_plane_walk_row_map_bit_for_bit
        return row_map_plane(N, plane) == plane and per == (plane + 1023) // 1024 and band % plane == 0
    raise ValueError(premise)
