"""Case table of the batched GCR's edge tests (a plain module, like tests/dist_worker.py — not a test file).

tests/test_multi_rhs_cases.py (CPU) runs every case through the oracle and asserts the premises — which step every column stops
at, what a zero right-hand side does; tests/test_gpu_multi_rhs_edges.py runs the same cases through mgcr_gcr_solve_multi and
asserts np.array_equal against `oracle_columns`.

The oracle's model of the batched solve (csrc/gcr_multi.hip, include/mgcr.h): grid of red_grid(n) workgroups, the operator's rows
associated as its layout says (lanes, CSR tail), lean restart cycles, the beta dots over the row map of the apply-embedding kernels
(oracle.row_map(n, reach)), and everything else — |b|^2, |r|^2, <r,Ap>, <Ap,Ap> of step 0 included — in the plain row order:
init_banded = xr_banded = False in every case.  The layout is PREDICTED on the host here (the arithmetic of csrc/spmv_layout.h
choose_width / choose_lanes) so that the table can be checked without a GPU; the GPU test asserts the prediction against
Operator.ell_layout().
"""
import functools
from collections import namedtuple

import numpy as np

from mgpreconditionedgcr_amd import problems
from oracle import oracle as orc

TAIL_CHUNK_CAP = 2048           # csrc: TAIL_CAP, what mgcr_op_ell_layout reports
PAT_MIN_ROWS = 1 << 15          # csrc/spmv_build.hip: below this no dictionary (and no stencil view) is tried
SHIFT = 0.1 + 0.05j

# ---- systems --------------------------------------------------------------------------------------------------------------------
# a system is a hashable tuple: (kind, ...).  `options`: library options the device operator is built under.
System = namedtuple("System", "kind N rowptr col val blocks nb bs")


@functools.lru_cache(maxsize=None)
def system(spec):
    kind = spec[0]
    if kind == "poisson":              # n^3
        N, _, rowptr, col, val = problems.poisson3d_csr(spec[1])
    elif kind == "slab":               # nz x n x n
        N, _, rowptr, col, val = problems.poisson3d_csr(spec[2], ni=spec[1])
    elif kind == "poisson_varied":     # the columns of n^3 Poisson, values that differ from row to row: dictionary form 2
        N, _, rowptr, col, val = problems.poisson3d_csr(spec[1])
        val = val * (1.0 + np.random.default_rng(3).uniform(0, 1, val.size))
    elif kind == "stencil9":           # 2-D 9-point constant-coefficient stencil on ny x nx: the stencil view with 9 slots
        N, rowptr, col, val = _stencil9(spec[1], spec[2])
    elif kind == "random":             # tests/test_gpu_bitwise.py test_irregular_spmv_bit_for_bit's matrices
        _, nrow, kw = spec
        rowptr, col, val = problems.random_csr(nrow, nrow, np.random.default_rng(nrow * 7 + nrow), **dict(kw))
        N = nrow
    elif kind == "skewed":             # test_banded_irregular_spmv_window_bit_for_bit's matrix
        _, N, window = spec
        rowptr, col, val = problems.skewed_csr(N, np.random.default_rng(window), window=window, long_rows=3, long_len=2500)
    elif kind == "bcsr":
        _, nb, bs = spec
        rows, cols, blocks = problems.unstructured_blocks(nb, bs)
        return System(kind, nb * bs, rows, cols, None, blocks, nb, bs)
    else:
        raise ValueError(spec)
    return System(kind, int(N), rowptr, col, val, None, 0, 0)


def _stencil9(ny, nx):
    j, i = np.meshgrid(np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    j, i = j.ravel(), i.ravel()
    r = j * nx + i
    masks, cols, vals = [], [], []
    for dj in (-1, 0, 1):              # ascending linear offset = ascending column
        for di in (-1, 0, 1):
            masks.append((j + dj >= 0) & (j + dj < ny) & (i + di >= 0) & (i + di < nx))
            cols.append(r + dj * nx + di)
            vals.append(8.0 if (dj, di) == (0, 0) else -1.0 + 0.125 * (dj + 2 * di))
    mask = np.stack(masks, axis=1)
    rowptr = np.zeros(r.size + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=rowptr[1:])
    return r.size, rowptr, np.stack(cols, axis=1)[mask], np.broadcast_to(np.array(vals, np.complex128), mask.shape)[mask]


@functools.lru_cache(maxsize=None)
def oracle_operator(spec, shift):
    s = system(spec)
    if s.kind == "bcsr":
        return orc.bcsr_from_triplets(s.nb, s.nb, s.bs, s.rowptr, s.col, s.blocks)
    A = orc.csr(s.N, s.N, s.rowptr, s.col, s.val)
    return orc.dirac(A, shift) if shift is not None else A


def host_layout(spec):
    """What Operator.ell_layout() will report for this system: csrc/spmv_layout.h choose_width (the width that minimises the bytes one
    apply streams) and choose_lanes.  reach: how far a dictionary's rows gather (0 where no dictionary is tried) — it matters through
    oracle.row_map only."""
    s = system(spec)
    lens = np.diff(s.rowptr)
    maxlen = int(lens.max())
    hist = np.bincount(lens, minlength=maxlen + 2).astype(np.int64)
    rows_ge = np.zeros(maxlen + 2, np.int64)
    rows_ge[:maxlen + 1] = np.cumsum(hist[:maxlen + 1][::-1])[::-1]
    tail = np.zeros(maxlen + 2, np.int64)
    tail[:maxlen] = np.cumsum(rows_ge[1:maxlen + 1][::-1])[::-1]
    W = np.arange(maxlen + 1)
    cost = 20. * W * float(s.N) + 40. * tail[:maxlen + 1] + 64. * rows_ge[1:maxlen + 2]
    w = int(np.argmin(cost))           # (the first minimum, like the loop's strict <)
    lanes = 1
    if not (w <= 8 or s.N >= 1 << 18):
        for L in (2, 4, 8, 16):
            if ((w + L - 1) // L * L - w) * 10 > w:
                continue
            lanes = L
            if s.N * L >= 1 << 17:
                break
    reach = 0
    if s.N >= PAT_MIN_ROWS and lanes == 1 and 1 <= w <= 32:
        reach = int(np.abs(s.col - np.repeat(np.arange(s.N), lens)).max())
    return dict(ell_width=w, lanes=lanes, tail_rows=int((lens > w).sum()), reach=reach, tail_chunk_cap=TAIL_CHUNK_CAP)


def device_order_of(spec):
    """The oracle's model of the batched solve on this system (module docstring); None for block-CSR, whose row sums the model cannot
    express."""
    s = system(spec)
    if s.kind == "bcsr":
        return None
    lay = host_layout(spec)
    band, per = orc.row_map(s.N, lay["reach"])
    lanes = lay["lanes"] > 1 or lay["tail_rows"] > 0
    return orc.device_order(blocks=0, band=band, per=per, init_banded=False, xr_banded=False,
                            ell_width=lay["ell_width"] if lanes else -1, ell_lanes=lay["lanes"], tail_cap=lay["tail_chunk_cap"],
                            lean=True, plane=orc.row_map_plane(s.N, lay["reach"]))


# ---- columns --------------------------------------------------------------------------------------------------------------------
# right-hand side columns: ("grid", seed) | ("zero",) | ("eig", modes) with modes = ((p, q, r), ...): the sum of these exact eigenvectors
# of n^3 Poisson, normalised.  x0 columns: ("grid", seed) scaled by 0.01 | ("zero",) | ("eigx0", modes): 0.25 A^-1 rhs formed per mode, so
# that r0 = b - A x0 keeps the direction of b (the stopping steps of the plain start carry over — checked, not assumed).
def _eig(n, modes, inverse=False):
    out = np.zeros(n ** 3, np.complex128)
    t = np.pi * np.arange(1, n + 1) / (n + 1)
    for p, q, r in modes:
        v = (np.sin(p * t)[:, None, None] * np.sin(q * t)[None, :, None] * np.sin(r * t)[None, None, :]).reshape(-1)
        lam = 6. - 2. * (np.cos(p * np.pi / (n + 1)) + np.cos(q * np.pi / (n + 1)) + np.cos(r * np.pi / (n + 1)))
        out += v / np.linalg.norm(v) / (lam if inverse else 1.)
    return out / np.sqrt(len(modes))


@functools.lru_cache(maxsize=None)
def column(spec, col):
    s = system(spec)
    if col[0] == "grid":
        return problems.rhs_grid(s.N, col[1])
    if col[0] == "x0grid":
        return 0.01 * problems.rhs_grid(s.N, col[1])
    if col[0] == "zero":
        return np.zeros(s.N, np.complex128)
    assert spec[0] == "poisson"
    if col[0] == "eig":
        return _eig(spec[1], col[1])
    if col[0] == "eigx0":
        return 0.25 * _eig(spec[1], col[1], inverse=True)
    raise ValueError(col)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# single: how the single solve relates — "rule" (include/mgcr.h: bit-identical), "small0" (bit-identical once the one-workgroup path is
# switched off with mgcr_set_small_solve_rows(0)), None (the single solve sums in another order: the oracle alone is the reference).
# stops: the step every column must stop at (None: max(max_iter, 1), nothing stops early).  options: library options for the build.
Case = namedtuple("Case", "id group spec shift restart max_iter tol use_x0 check_every rhs x0 stops single bits options expect")
P16, P17 = ("poisson", 16), ("poisson", 17)


def _case(id, group, spec, restart, max_iter, tol, rhs, x0=None, shift=None, check_every=0, stops=None, single="rule", bits=True,
          options=(), expect=None):
    return Case(id, group, spec, shift, restart, max_iter, tol, x0 is not None, check_every, tuple(rhs), None if x0 is None else tuple(x0),
                stops, single, bits, tuple(options), expect)


def grid_cols(k, seed0=1):
    return [("grid", seed0 + j) for j in range(k)]


def x0_cols(k):
    return [("x0grid", 7 + j) for j in range(k)]


# a. cycles: every (restart, max_iter) pair at k = 1, 2, 16 (column groups of 1, 2 and 4 columns) and at one of the ragged k = 3, 5, 13 (a
# partly masked last group of 4) in turn; 16^3 (4 workgroups) and 17^3 (a ragged last workgroup) in turn.  tol 0 and 1e-30 in turn.
CYCLE_PAIRS = [(1, 1), (1, 2), (1, 7), (2, 1), (2, 2), (2, 3), (2, 5), (3, 2), (3, 3), (3, 4), (3, 7), (5, 0), (5, 1), (5, 4), (5, 5), (5, 6),
               (5, 11), (8, 7), (8, 8), (8, 9), (8, 17), (15, 15), (15, 16), (16, 15), (16, 16), (16, 17), (16, 33), (20, 10), (17, 15)]
RAGGED = (3, 5, 13)
UNSUPPORTED = [(17, 16), (40, 40)]


def _cycles():
    out = []
    for i, (restart, max_iter) in enumerate(CYCLE_PAIRS):
        spec = (P16, P17)[i % 2]
        for k in (1, 2, RAGGED[i % 3], 16):
            out.append(_case("cycle-r%d-m%d-k%d-n%d" % (restart, max_iter, k, spec[1]), "cycles", spec, restart, max_iter, (0.0, 1e-30)[i % 2],
                             grid_cols(k)))
    # solves that do converge: restart 1 (every step closes), 3, 16 (the full table), ragged k, stops in the middle of the batch
    for restart, k, tol, spec in ((1, 5, 0.01, P16), (3, 13, 0.01, P17), (16, 3, 0.01, P16)):
        out.append(_case("cycle-converges-r%d-k%d" % (restart, k), "cycles", spec, restart, 60, tol, grid_cols(k), expect="converges"))
    return out


# b. freezing: restart 4; columns that stop at steps 1, 3, 4 (a closing step), 5 (one step after it), 8, and a zero right-hand side.
# sums of m eigenvectors with well separated eigenvalues stop at step m <= restart; the later stops come from tight clusters of
# eigenvalues.  (chosen by running the oracle over candidates; tests/test_multi_rhs_cases.py asserts the steps)
FREEZE_TOL = 1e-4
FREEZE_MODES = {}      # step -> modes, filled below
FREEZE_STEPS = (1, 3, 4, 5, 8)


def _freeze():
    out = []
    n = 16
    cols = [("eig", FREEZE_MODES[s]) for s in FREEZE_STEPS]
    x0s = [("eigx0", FREEZE_MODES[s]) for s in FREEZE_STEPS]
    for use_x0 in (False, True):
        for ce in (1, 3, 0):
            out.append(_case("freeze-k6-ce%d-x0%d" % (ce, use_x0), "freeze", ("poisson", n), 4, 40, FREEZE_TOL, cols + [("zero",)],
                             x0=x0s + [("zero",)] if use_x0 else None, check_every=ce, stops=FREEZE_STEPS + (1,)))
            out.append(_case("freeze-k5-reversed-ce%d-x0%d" % (ce, use_x0), "freeze", ("poisson", n), 4, 40, FREEZE_TOL, cols[::-1],
                             x0=x0s[::-1] if use_x0 else None, check_every=ce, stops=FREEZE_STEPS[::-1]))
    return out


# c. use_x0 through every apply form: restart 3, max_iter 7, tol 0, k = 3, 8, 13
X0_FORMS = [
    # id, system, shift, options, single, bits
    ("slab-1lane", P16, None, (), "rule", True),
    ("multi-lane-700", ("random", 700, (("min_len", 30), ("max_len", 45))), None, (), "small0", True),
    ("tail-long-rows-6000", ("random", 6000, (("min_len", 1), ("max_len", 7), ("long_rows", 7), ("long_len", 3000))), None, (), "rule", True),
    ("lds-window-70000", ("skewed", 70000, 300), None, (), "rule", True),
    ("dictionary-1", ("poisson", 32), None, (("stencil_storage", 0),), "rule", True),
    ("dictionary-2", ("poisson_varied", 32), None, (), "rule", True),
    ("stencil-7", ("poisson", 32), None, (), "rule", True),
    ("stencil-9", ("stencil9", 182, 182), None, (), "rule", True),
    ("dirac-slab", P16, SHIFT, (), "rule", True),
    ("dirac-stencil", ("poisson", 32), SHIFT, (), "rule", True),
    ("block-csr-20", ("bcsr", 600, 20), None, (), "rule", False),
]
# what the GPU test asserts of the storage each form must take (Operator.storage_format()[0], lanes > 1, tail rows, x_window)
X0_STORAGE = {"slab-1lane": dict(fmt=0, lanes=1, tail=False), "multi-lane-700": dict(fmt=0, lanes_gt1=True), "tail-long-rows-6000": dict(fmt=0, tail=True),
              "lds-window-70000": dict(fmt=0, tail=True, window=1024), "dictionary-1": dict(fmt=1), "dictionary-2": dict(fmt=2),
              "stencil-7": dict(fmt=3, slots=7), "stencil-9": dict(fmt=3, slots=9), "dirac-slab": dict(fmt=0, lanes=1, tail=False),
              "dirac-stencil": dict(fmt=3, slots=7), "block-csr-20": dict()}


def _x0_forms():
    out = []
    for tag, spec, shift, options, single, bits in X0_FORMS:
        for k in (3, 8, 13):
            out.append(_case("x0-%s-k%d" % (tag, k), "x0", spec, 3, 7, 0.0, grid_cols(k), x0=x0_cols(k), shift=shift, single=single, bits=bits,
                             options=options))
    return out


# d. plain-order territory: where the single solve sums in another order, so only the oracle can be the reference
KIND2_NZ = 8      # 8 x 256 x 256 = 512 x 1024 rows: the smallest slab with a full grid, whose bands are one plane wide (xr_fuse_kind 2)


def _plain_order():
    out = []
    for use_x0 in (False, True):
        out.append(_case("kind2-slab-x0%d" % use_x0, "plain", ("slab", KIND2_NZ, 256), 5, 7, 0.0, grid_cols(3), x0=x0_cols(3) if use_x0 else None,
                         single=None))
    for n in (8, 10):      # 512 and 1000 rows, the small-solve limit at its default
        for k in (2, 5):
            out.append(_case("small-%d-k%d" % (n ** 3, k), "plain", ("poisson", n), 3, 9, 0.0, grid_cols(k), single=None))
    return out


# e. reuse of the work storage: one GCR object, this sequence (the first and the last are the same solve)
def _reuse():
    cols = [("eig", FREEZE_MODES[s]) for s in (8, 1, 5, 3, 4)]
    stops = (8, 1, 5, 3, 4)
    first = _case("reuse-1-k5-r5-m40-freezing", "reuse", P16, 5, 40, FREEZE_TOL, cols, stops=stops)
    return [first,
            _case("reuse-2-k5-r5-m6", "reuse", P16, 5, 6, 0.0, grid_cols(5)),
            _case("reuse-3-k3-r5-m6", "reuse", P16, 5, 6, 0.0, grid_cols(3)),
            _case("reuse-4-k5-r2-m6", "reuse", P16, 2, 6, 0.0, grid_cols(5)),
            first._replace(id="reuse-5-first-again")], stops


def _modes_window(n, start, m):
    """m modes (p, q, r), p <= q <= r, with consecutive distinct eigenvalues starting at rank `start` of the sorted spectrum."""
    c = np.cos(np.pi * np.arange(1, n + 1) / (n + 1))
    lam = sorted((round(6. - 2. * (c[p - 1] + c[q - 1] + c[r - 1]), 12), (p, q, r)) for p in range(1, n + 1) for q in range(p, n + 1) for r in range(q, n + 1))
    out, last = [], None
    for l, mode in lam:
        if l != last:
            out.append(mode)
            last = l
    return tuple(out[start:start + m])


FREEZE_MODES.update({
    1: ((3, 5, 7),),
    3: ((1, 1, 1), (8, 8, 8), (16, 16, 16)),
    4: ((1, 2, 3), (6, 7, 8), (11, 12, 13), (16, 16, 15)),
    5: _modes_window(16, 5, 8),
    8: _modes_window(16, 1, 11),
})


def all_cases():
    reuse, _ = _reuse()
    return _cycles() + _freeze() + _x0_forms() + _plain_order() + reuse


def reuse_sequence():
    return _reuse()[0]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_column(spec, shift, restart, max_iter, tol, use_x0, rhs, x0):
    model = device_order_of(spec)
    A = oracle_operator(spec, shift)
    p = orc.gcr_param(restart=restart, max_iter=max_iter, tol=tol, use_x0=use_x0)
    b = column(spec, rhs)
    x0v = column(spec, x0) if x0 is not None else None
    if model is None:
        with orc.device_order(lean=True):
            return orc.gcr_solve(A, p, b, x0v)
    with model:
        return orc.gcr_solve(A, p, b, x0v)


def oracle_columns(case):
    """[(x, history, iterations, converged)] per column of the case, the oracle in the batched solve's summation order (columns are
    independent: a column of one case is the same solve as that column of another, and is computed once)."""
    return [_oracle_column(case.spec, case.shift, case.restart, case.max_iter, case.tol, case.use_x0, case.rhs[j],
                           case.x0[j] if case.x0 is not None else None) for j in range(len(case.rhs))]
