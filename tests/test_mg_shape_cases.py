"""CPU check of the multigrid shape cases (tests/mg_shape_cases.py): the premises tests/test_gpu_mg_shapes.py relies on.  Every case
is shown to be what its row of the table says, the oracle is compared with the independent extended-precision model within the a-priori
rounding bound of a double sum and, at block edge 4, with the real reference's golden; three mutants of the model show that the
comparisons see the errors the kernels could make.  No case is skipped: a case whose premise fails is a failing test.

MGCR_MG_SHAPES_OBSERVED=<file> writes the largest observed ratios to the bound anew (tests/golden/observed_mg_shapes.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import mg_shape_cases as ms

CASES, IDS = ms.CASES, ms.IDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ms.GOLDEN, "observed_mg_shapes.json")
_seen = {}


def _level0(case):
    p = ms.problem(case)
    agg, nagg = ms.model_aggregates(case.dims, case.blocked, case.sub)
    return p, agg, nagg, ms.members(agg, nagg)


def test_extended_precision_is_extended():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_table_is_the_issues():
    assert len(set(IDS)) == len(IDS)
    want = {"edge3": ((9, 9, 9), (1, 1, 1), 3, 2, 2), "edge4-pairs": ((8, 8, 8), (1, 1, 1), 4, 1, 1),
            "edge4-unblocked": ((8, 8, 3), (1, 1, 0), 4, 3, 1), "edge4-two-level": ((16, 16, 2), (1, 1, 0), 4, 2, 2),
            "triples": ((8, 8, 3), (1, 1, 0), 2, 1, 1), "ne6": ((4, 4, 4, 3), (1, 1, 1, 0), 2, 6, 1),
            "nbr-regrow-1": ((200, 12), (1, 0), 2, 1, 1), "tail": ((250, 12), (1, 0), 2, 1, 1),
            "dict-offsets": ((32, 32, 32), (1, 1, 1), 4, 1, 1), "sample-edge4": ((4, 4, 4, 4, 4, 3), (1, 1, 1, 1, 0, 0), 4, 4, 1)}
    for id, row in want.items():
        c = ms.BY_ID[id]
        assert (c.dims, c.blocked, c.sub, c.ne, c.levels) == row, id
    for id in ("edge3-const", "edge3-pairs", "nbr-regrow-2", "block-op"):      # the rows the issue left to be shaped
        assert id in ms.BY_ID
    assert ms.BY_ID["edge3-const"].sub == 3 and ms.BY_ID["edge3-const"].vec == "const" and ms.BY_ID["dict-offsets"].vec == "const"
    assert ms.BY_ID["nbr-regrow-2"].shift is not None and ms.BY_ID["sample-edge4"].shift == 0.1
    assert ms.BY_ID["tail"].op == ("random", 1, 6, 5, 900) and ms.BY_ID["nbr-regrow-1"].op[:3] == ("random", 6, 12)
    assert ms.BY_ID["block-op"].op[0] == "blocks" and ms.BY_ID["block-op"].blocked == (1, 0)
    assert max(c.ne for c in CASES) == 6                                       # gs_kernel / gal_fill_kernel past 4 vectors
    assert 32 ** 3 == 1 << 15                                                  # csrc/spmv_build.hip PAT_MIN_ROWS: the smallest dictionary


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_shape_premises(case):
    p, agg, nagg, mem = _level0(case)
    S = mem.shape[1]
    paired = [[ms.batch_is_paired(b) for b in ms.batches(mem[a])] for a in range(nagg)]
    full = S // ms.BATCH
    sizes = {"edge3": (27, 27), "edge3-const": (9, 27), "edge3-pairs": (9, 27), "edge4-pairs": (8, 64), "edge4-unblocked": (4, 48),
             "edge4-two-level": (16, 32), "triples": (16, 12), "ne6": (8, 24), "nbr-regrow-1": (100, 24), "nbr-regrow-2": (300, 16),
             "tail": (125, 24), "dict-offsets": (512, 64), "block-op": (100, 12), "sample-edge4": (1, 3072)}
    assert (nagg, S) == sizes[case.id]
    assert [np.prod(d) for d, _ in ms.level_meshes(case)][0] == p.N
    Mo = ms.oracle_mg(case)
    assert [Mo.level_dim(l) for l in range(case.levels + 1)] == {"edge3": [729, 54, 2], "edge4-two-level": [512, 32, 2]}.get(
        case.id, [p.N, nagg * case.ne])
    if case.id.startswith("edge3"):
        assert S % ms.BATCH == 3 and full == 3                                 # three full batches + 3
    if case.id == "edge3":
        # level 1 is the lattice of aggregates x 2 vectors, ONE aggregate of 54 members, and the coarsest level has 2 unknowns
        (d1, b1) = ms.level_meshes(case)[1]
        assert (d1, b1) == ((3, 3, 3, 2), (1, 1, 1, 0))
        a1, n1 = ms.model_aggregates(d1, b1, case.sub)
        assert n1 == 1 and a1.size == 54 and 54 % ms.BATCH == 6
        assert not any(any(row) for row in paired)                             # runs of three members: test_runs_of_three_never_pair
    if case.id == "edge4-two-level":
        (d1, b1) = ms.level_meshes(case)[1]
        assert (d1, b1) == ((4, 4, 2), (1, 1, 0)) and ms.model_aggregates(d1, b1, case.sub)[1] == 1
    if case.id in ("edge3-const", "edge3-pairs"):
        # one vector per aggregate, so the device takes the 32-byte loads where the condition holds: aggregates with paired AND unpaired
        # full batches, and aggregates none of whose batches pairs although they hold adjacent rows — pairs that start on an odd row
        assert case.ne == 1
        assert any(any(row[:full]) and not all(row[:full]) for row in paired)
        odd = [a for a in range(nagg) if not any(paired[a]) and any(ms.odd_start_pairs(b) for b in ms.batches(mem[a])[:full])]
        assert odd
        assert all(not row[full] for row in paired)                            # the partial batch never pairs
    if case.id in ("edge4-pairs", "dict-offsets"):
        assert case.ne == 1 and all(all(row) for row in paired) and S % ms.BATCH == 0
    if case.id == "triples":
        # 12 members = 2 x 2 sites of 3: the first batch is paired although its pairs straddle sites (3 is odd), then a batch of 4
        assert case.ne == 1 and all(row == [True, False] for row in paired) and S - ms.BATCH == 4
        first = mem[0][:ms.BATCH]
        assert any(first[u] // 3 != first[u + 1] // 3 for u in range(0, ms.BATCH, 2))
    if case.id == "edge4-unblocked":
        assert case.ne == 3 and S == 48
    if case.id == "ne6":
        assert case.ne == 6 and S >= case.ne
    if case.id == "sample-edge4":
        assert nagg == 1 and S == 3072 and p.shift == 0.1 and (np.diff(p.rowptr) == 39).all()
    if case.id == "tail":
        lens = np.diff(p.rowptr)
        assert (lens > 400).sum() == 5 and np.sort(lens)[-6] <= 7              # five rows far longer than any ELL width that pays
    if case.id == "block-op":
        nb, bs, rows, cols, blocks = p.triplets
        assert (nb, bs) == case.dims and case.blocked == (1, 0)                # aggregates of `sub` block rows, bs unblocked
        x = ms.problems.rhs_grid(p.N, 1)
        dense = np.zeros((p.N, p.N), np.complex128)
        for r, c, b in zip(rows, cols, blocks):
            dense[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs] += b
        y = ms.oracle_fine(p)(x)
        assert np.abs(dense @ x - y).max() <= 1e-13 * np.abs(y).max()          # blocks_as_csr is the block operator
    if case.id == "dict-offsets":
        # 27 distinct rows of column offsets (a 32^3 box), every entry its own value: the values cannot go into a dictionary
        rows = np.repeat(np.arange(p.N), np.diff(p.rowptr))
        assert np.unique(p.val).size == p.val.size and np.unique(p.col - rows).size == 7
    # the neighbour lists gal_count_kernel has to hold
    cnt = ms.neighbour_counts(p.rowptr, p.col, agg, nagg, p.shift)
    lo, hi = {"first": (0, ms.MAXNB_FIRST), "regrow1": (ms.MAXNB_FIRST, ms.MAXNB_FIRST * ms.MAXNB_GROWTH),
              "regrow2": (ms.MAXNB_FIRST * ms.MAXNB_GROWTH, ms.MAXNB_FIRST * ms.MAXNB_GROWTH ** 2)}[case.nbr]
    assert lo < cnt.max() <= hi, cnt.max()
    assert {c.id for c in CASES if c.nbr == "regrow1"} == {"nbr-regrow-1", "tail", "block-op"}
    assert {c.id for c in CASES if c.nbr == "regrow2"} == {"nbr-regrow-2"}
    # ... which the oracle's coarse operator has (a block per neighbour): the count of level 1's dense view
    if case.ne == 1 and case.nbr != "first":
        Ac = ms.dense_view(ms.oracle_mg(case).level_op(1), nagg)
        assert (Ac != 0).sum(axis=1).max() == cnt.max()


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    """tests/cpp/spmv_layout_check.cpp — the host decisions of the Sparse format build (csrc/spmv_layout.h) — built as
    tests/test_spmv_layout.py builds it; `split` mode: the width, lanes and tail of a row-length histogram"""
    exe = str(tmp_path_factory.mktemp("mg_shapes_layout") / "spmv_layout_check")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "spmv_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr

    def split(rowptr):
        lens, counts = np.unique(np.diff(rowptr), return_counts=True)
        p = subprocess.run([exe, "split"] + ["%d:%d" % lc for lc in zip(lens, counts)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, p.stdout + p.stderr
        words = p.stdout.split()
        assert words[0] == "split"
        return {k: int(v) for k, v in (w.split("=") for w in words[1:])}

    return split


def test_how_the_build_splits_the_scalar_operators(layout_check):
    """`tail`: the five long rows leave the slab with all but a handful of their entries — the Galerkin kernels read hundreds of
    entries per row through for_each_entry's search in trows.  (The width that streams the fewest bytes also sends the last entry or two
    of the longest SHORT rows to the tail, here and in most random cases: tail rows of one entry were reached before, long ones not.)
    The two regrowth cases' rows (up to 13 and 51 entries) and the sample's (39) are dealt to several lanes: for_each_entry walks the
    lane-interleaved slab.  (The device objects are asked again in tests/test_gpu_mg_shapes.py.)"""
    got = {c.id: layout_check(ms.problem(c).rowptr) for c in CASES if c.op[0] != "blocks"}
    assert all(s["nrow"] == ms.problem(ms.BY_ID[i]).N for i, s in got.items())
    tail = got["tail"]
    lens = np.diff(ms.problem(ms.BY_ID["tail"]).rowptr)
    assert tail["W"] <= 7 and tail["tail_rows"] >= 5 and tail["tail_nnz"] >= np.sort(lens)[-5:].sum() - 5 * tail["W"] > 2000
    assert all(s["tail_nnz"] <= 2 * s["tail_rows"] for i, s in got.items() if i not in ("tail", "nbr-regrow-2"))
    assert got["nbr-regrow-1"]["lanes"] > 1 and got["nbr-regrow-2"]["lanes"] > 1 and got["sample-edge4"]["lanes"] > 1
    assert got["dict-offsets"]["tail_nnz"] == 0
    assert got["dict-offsets"]["lanes"] == 1 and got["dict-offsets"]["W"] == 7          # what the dictionary needs (spmv_build.hip)


@pytest.mark.parametrize("dims", [(9, 9, 9), (9, 9, 6), (6, 3, 12)])
def test_runs_of_three_never_pair(dims):
    """all dimensions blocked with edge 3: an aggregate's members come in runs of 3 consecutive rows, so positions 2 and 3 of a batch
    of 8 are never adjacent rows — no batch is four adjacent pairs, whatever the mesh (why edge3-const unblocks its fastest dimension)"""
    agg, nagg = ms.model_aggregates(dims, (1, 1, 1), 3)
    mem = ms.members(agg, nagg)
    assert not any(ms.batch_is_paired(b) for a in range(nagg) for b in ms.batches(mem[a]))
    assert any(ms.odd_start_pairs(b) for a in range(nagg) for b in ms.batches(mem[a]))


def _oracle_vs_model(case):
    """the oracle's hierarchy against the model, level by level -> {piece: largest ratio to the bound}"""
    p = ms.problem(case)
    Mo = ms.oracle_mg(case)
    out = {}
    rowptr, col, val, shift, vecs = p.rowptr, p.col, p.val, p.shift, p.vecs
    for l, (dims, blocked) in enumerate(ms.level_meshes(case)):
        agg, nagg = ms.model_aggregates(dims, blocked, case.sub)
        pvo, aggo = Mo.prolongator(l)
        assert np.array_equal(agg, aggo), (case.id, l)
        n, nc = agg.size, nagg * case.ne
        assert Mo.level_dim(l) == n and Mo.level_dim(l + 1) == nc
        pvm, bound = ms.model_prolongator(agg, nagg, vecs, pvo)
        out["prolongator-%d" % l] = ms.ratio(pvo, pvm, bound)
        x = ms.problems.rhs_grid(n, 7)
        Rx = Mo.restrict(l, x)
        out["restrict-%d" % l] = ms.ratio(Rx, *ms.model_restrict(agg, nagg, pvo, x))
        out["expand-%d" % l] = ms.ratio(Mo.expand(l, Rx), *ms.model_expand(agg, pvo, Rx))
        Aco = ms.dense_view(Mo.level_op(l + 1), nc)
        Acm, bound = ms.model_galerkin(rowptr, col, val, agg, nagg, pvo, shift)
        assert not Aco[bound == 0].any()                                       # no entry where the model has no term
        out["galerkin-%d" % l] = ms.ratio(Aco, Acm, bound)
        # the next level: the oracle's coarse operator and restricted vectors, which the lines above have just checked
        vecs = np.array([Mo.restrict(l, v) for v in vecs])
        rowptr, col, val = ms.csr_of_dense(Aco)
        shift = None
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_is_the_model_within_the_rounding_bound(case):
    got = _oracle_vs_model(case)
    _seen[case.id] = got
    assert set(got) == {"%s-%d" % (piece, l) for piece in ("prolongator", "restrict", "expand", "galerkin") for l in range(case.levels)}
    assert all(r <= 1.0 for r in got.values()), got


def test_observed_ratios_are_recorded():
    """tests/golden/observed_mg_shapes.json holds the largest ratio to the bound per case and piece, as first observed"""
    target = os.environ.get("MGCR_MG_SHAPES_OBSERVED")
    if target:
        seen = {c.id: _seen.get(c.id) or _oracle_vs_model(c) for c in CASES}
        with open(target, "w") as f:
            json.dump({"bound": "(t + 4) * 2^-53 * sum |terms|, entrywise", "largest_ratio": seen}, f, indent=1, sort_keys=True)
            f.write("\n")
    rec = json.load(open(OBSERVED))["largest_ratio"]
    assert set(rec) == set(IDS)
    for c in CASES:
        assert len(rec[c.id]) == 4 * c.levels and all(0 <= r <= 1.0 for r in rec[c.id].values()), c.id


def test_oracle_is_the_real_reference_at_edge_4():
    """tests/golden/mg_4x4_edge4.npz: the reference's own MG on the 4x4 sample with subblock_dim 4 — one block of all 256 sites, 3072
    unknowns, 4 vectors.  Block map, every prolongator column and R v bit for bit; P R v and A_c to test_g9_mg_pieces' tolerances."""
    g = ms.golden_edge4()
    case = ms.BY_ID["sample-edge4"]
    p = ms.problem(case)
    assert (int(g["nblocks"]), int(g["block_size"]), int(g["ne"]), int(g["sub"])) == (1, 256, 4, 4)
    agg, nagg = orc.mg_aggregates(case.dims, case.blocked, case.sub)
    assert nagg == 1 and not agg.any()
    assert np.array_equal(np.sort(g["block_map"][0]), np.arange(256))          # sites (12 unknowns each): the one block holds them all
    assert set(np.unique(np.arange(3072)[agg == 0] // 12)) == set(g["block_map"][0])
    pv = orc.mg_prolongator(agg, nagg, p.vecs)
    for k in range(4):
        assert np.array_equal(pv[:, k], g["P"][0, k]), k
    Rv = orc.mg_restrict(agg, nagg, pv, g["v"])
    assert np.array_equal(Rv, g["Rv"])
    assert np.allclose(orc.mg_expand(agg, pv, Rv), g["PRv"], rtol=0, atol=1e-15)
    rows, cols, blocks = orc.mg_galerkin(p.rowptr, p.col, p.val, agg, nagg, pv, shift=float(g["k"]))
    assert rows.tolist() == [0] and cols.tolist() == [0]
    ref = g["Ac_dense"]
    assert np.abs(blocks[0] - ref).max() <= 1e-15 * np.abs(ref).max()
    H = orc.bcsr_from_triplets(1, 1, 4, rows, cols, blocks)
    assert np.abs(H(Rv) - g["AcRv"]).max() <= 1e-14 * np.abs(g["AcRv"]).max()
    # ... and the hierarchy the GPU test compares the device with is made of these pieces
    Mo = ms.oracle_mg(case)
    pvo, aggo = Mo.prolongator(0)
    assert np.array_equal(pvo, pv) and np.array_equal(aggo, agg) and np.array_equal(Mo.restrict(0, g["v"]), Rv)
    assert np.array_equal(ms.dense_view(Mo.level_op(1), 4), blocks[0])


# ---- mutants: the comparisons see the errors these kernels could make -----------------------------------------------------------
def _restrict_ratio(case, mutant):
    p, agg, nagg, _ = _level0(case)
    Mo = ms.oracle_mg(case)
    pvo, _ = Mo.prolongator(0)
    x = ms.problems.rhs_grid(p.N, 7)
    return ms.ratio(Mo.restrict(0, x), *ms.model_restrict(agg, nagg, pvo, x, mutant=mutant))


def test_a_restrict_that_drops_the_members_after_the_last_full_batch_is_seen():
    broken = [c.id for c in CASES if _restrict_ratio(c, "drop-tail") > 1e3]
    assert {"edge3", "edge3-const", "edge3-pairs", "triples"} <= set(broken), broken
    whole = [c.id for c in CASES if ms.members(*ms.model_aggregates(c.dims, c.blocked, c.sub)).shape[1] % ms.BATCH == 0]
    assert not set(broken) & set(whole) and all(_restrict_ratio(ms.BY_ID[i], None) <= 1.0 for i in broken)


def test_a_restrict_that_swaps_the_members_of_odd_start_pairs_is_seen():
    broken = [c.id for c in CASES if _restrict_ratio(c, "swap-odd-pairs") > 1e3]
    assert {"edge3", "edge3-pairs"} <= set(broken), broken
    assert "edge4-pairs" not in broken and "dict-offsets" not in broken         # (their pairs all start on even rows)
    # under a constant prolongator the swap only reorders a sum of equal weights: edge3-const cannot see it — edge3-pairs, the same
    # mesh with a random vector, is in the table for that
    assert "edge3-const" not in broken


def test_a_galerkin_product_whose_neighbour_lists_stop_at_64_is_seen():
    broken = []
    for c in CASES:
        if c.levels != 1 or c.id == "dict-offsets":        # (level 0 of the others; 32^3 has 7 neighbours and the largest product)
            continue
        p, agg, nagg, _ = _level0(c)
        Mo = ms.oracle_mg(c)
        pvo, _ = Mo.prolongator(0)
        Aco = ms.dense_view(Mo.level_op(1), nagg * c.ne)
        Acm, bound = ms.model_galerkin(p.rowptr, p.col, p.val, agg, nagg, pvo, p.shift, cut=ms.MAXNB_FIRST)
        if (Aco[bound == 0] != 0).any() or ms.ratio(Aco, Acm, bound) > 1e3:
            broken.append(c.id)
    assert sorted(broken) == sorted(c.id for c in CASES if c.nbr != "first"), broken
