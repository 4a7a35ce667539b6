"""Premises of the even-odd hopping-parameter scan's tests, checked with numpy alone on the models of tests/evenodd_cases.py: where
each column of the ladder stops, that every stopped column reconstructs to a solution of the FULL system, and that the bipartite
cases are what tests/evenodd_multi_cases.py says they are."""
import numpy as np
import pytest

from tests import evenodd_cases as ec
from tests import evenodd_multi_cases as emc


@pytest.fixture(scope="module")
def ladder():
    c, p = ec.case("sample"), ec.case_plan("sample")
    b = ec.rhs(c.n)
    out = []
    for k in emc.LADDER:
        bhat = ec.prepare(p, k, b)
        xe, hist, it, conv = ec.gcr(lambda v: ec.schur_apply(p, k, v), bhat, emc.LADDER_RESTART, emc.LADDER_TOL, emc.LADDER_MAX_ITER)
        out.append(dict(k=k, b=b, x=ec.reconstruct(p, k, b, xe), it=it, conv=conv))
    return out


def test_the_ladder_stops_at_five_distinct_steps_and_once_at_the_cap(ladder):
    its = [s["it"] for s in ladder]
    assert its == emc.LADDER_MODEL_STOPS
    assert len(set(its)) == len(its) and its.count(emc.LADDER_MAX_ITER) == 1
    assert [s["conv"] for s in ladder] == [True] * 5 + [False]


def test_every_stopped_column_solves_the_full_system(ladder):
    c = ec.case("sample")
    for s in ladder:
        if s["conv"]:
            r = ec.dirac_apply(c, s["k"], s["x"]) - s["b"]
            assert np.linalg.norm(r) / np.linalg.norm(s["b"]) <= 1e-10, s["k"]


def test_shifts_are_distinct_and_partly_complex():
    for name in ("sample", "chain", "long"):
        ks = emc.shifts(name, 16)
        assert len(set(ks)) == 16 and any(z.imag != 0 for z in ks) and any(z.imag == 0 for z in ks) and all(z != 0 for z in ks)


@pytest.mark.parametrize("name", list(emc.BIPARTITE))
def test_bipartite_cases_have_the_given_parity_and_blocks(name):
    c, par = emc.bipartite_case(name)
    A, B = emc.bipartite_blocks(name)
    assert ec.first_conflict(c.n, c.rowptr, c.col, par) is None
    p = emc.case_plan(name)
    n = emc.BIPARTITE[name][0]
    assert p.even.size == p.odd.size == n
    for half, blk in ((p.eo, A), (p.oe, B)):
        assert half[:2] == (n, n)
        assert np.array_equal(half[2], blk[0]) and np.array_equal(half[3], blk[1]) and np.array_equal(half[4], blk[2])
