"""CPU check of the batched GCR's case table (tests/multi_rhs_cases.py): every case runs through `oracle_columns` and must have the
premises tests/test_gpu_multi_rhs_edges.py relies on — the step each column stops at, what a zero right-hand side does, finite numbers
everywhere else.  No case is skipped: a case whose premise fails is a failing test."""
import numpy as np
import pytest

from tests import multi_rhs_cases as mc

CASES = mc.all_cases()


def test_table_covers_what_it_must():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    cyc = [c for c in CASES if c.group == "cycles" and c.expect is None]
    pairs = {(c.restart, c.max_iter) for c in cyc}
    assert pairs == set(mc.CYCLE_PAIRS) and len(mc.CYCLE_PAIRS) == 29
    for pair in pairs:      # every pair sees a group of 1, of 2, a full and a ragged group of 4
        ks = {len(c.rhs) for c in cyc if (c.restart, c.max_iter) == pair}
        assert {1, 2, 16} <= ks and ks & set(mc.RAGGED), (pair, ks)
    for k in (1, 2, 3, 5, 13, 16):
        assert len({(c.restart, c.max_iter) for c in cyc if len(c.rhs) == k}) >= 4, k
    assert {c.spec for c in cyc} == {mc.P16, mc.P17}
    assert {c.restart for c in CASES if c.expect == "converges"} == {1, 3, 16}
    fr = [c for c in CASES if c.group == "freeze"]
    assert {(len(c.rhs), c.check_every, c.use_x0) for c in fr} == {(k, ce, x) for k in (5, 6) for ce in (0, 1, 3) for x in (False, True)}
    assert all(c.restart == 4 and sorted(c.stops[:5]) == [1, 3, 4, 5, 8] for c in fr)
    x0 = [c for c in CASES if c.group == "x0"]
    assert all(c.use_x0 and (c.restart, c.max_iter, c.tol) == (3, 7, 0.0) for c in x0)
    assert {(c.id.rsplit("-k", 1)[0][3:], len(c.rhs)) for c in x0} == {(f[0], k) for f in mc.X0_FORMS for k in (3, 8, 13)}
    seq = mc.reuse_sequence()
    assert [(len(c.rhs), c.restart, c.max_iter) for c in seq] == [(5, 5, 40), (5, 5, 6), (3, 5, 6), (5, 2, 6), (5, 5, 40)]


def test_host_layout_of_the_small_shapes():
    """the layouts the oracle's model is built from (asserted against the device's own on the GPU)"""
    lay = mc.host_layout(mc.P16)
    assert (lay["ell_width"], lay["lanes"], lay["tail_rows"]) == (7, 1, 0)
    lay = mc.host_layout(mc.X0_FORMS[1][1])
    assert lay["lanes"] > 1
    lay = mc.host_layout(mc.X0_FORMS[2][1])
    assert lay["lanes"] == 1 and lay["tail_rows"] > 0
    N = mc.KIND2_NZ * 256 * 256
    band, per = mc.orc.row_map(N, mc.host_layout(("slab", mc.KIND2_NZ, 256))["reach"])
    assert (band, per) == (256 * 256, 64) and mc.orc.row_map(N - 256 * 256, 256 * 256)[1] != 64    # one plane less: no band is a plane wide


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_premises(case):
    cols = mc.oracle_columns(case)
    assert len(cols) == len(case.rhs)
    full = max(case.max_iter, 1)
    its = [c[2] for c in cols]
    for j, (x, hist, it, conv) in enumerate(cols):
        assert hist.size == it + 1 and conv == (it != case.max_iter)
        if case.rhs[j] == ("zero",):
            # what tests/test_gpu_parity.py test_zero_rhs_behaves_like_the_reference expects of the single solve: 0 / 0 is NaN, the
            # loop's comparison is false: one iteration, reported as converged, NaN in the history
            assert it == 1 and conv and np.isnan(hist[1])
            continue
        assert np.isfinite(hist).all() and np.isfinite(x).all(), (case.id, j)
        if case.stops is not None:
            assert it == case.stops[j], (case.id, j, it, hist[max(it - 1, 0):])
        elif case.expect is None:
            assert it == full, (case.id, j, it)
    if case.stops is not None:
        assert max(its) < case.max_iter
    if case.expect == "converges":
        assert max(its) < case.max_iter and len(set(its)) > 1, its      # every column stops, and not all at the same step
