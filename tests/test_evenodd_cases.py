"""Premises of the even-odd tests, checked with numpy alone on the model of tests/evenodd_cases.py: the golden 4^4 matrix is a pure
hopping matrix whose two-colouring is the site parity; the Schur solve reconstructs to the full system's solution with the residual
the mapped history entry predicts; and it takes fewer steps than the full solve."""
import numpy as np
import pytest

from tests import evenodd_cases as ec

TOL = 1e-10


def test_sample_is_bipartite_and_coloured_by_site_parity():
    c = ec.case("sample")
    par = ec.colour(c.n, c.rowptr, c.col)
    assert ec.first_conflict(c.n, c.rowptr, c.col, par) is None          # no entry joins rows of equal colour, no diagonal
    assert c.col.size == 119808
    assert np.array_equal(par, ec.sample_site_parity())
    p = ec.case_plan("sample")
    assert p.even.size == p.odd.size == 1536


@pytest.mark.parametrize("name", ["open4d", "chain", "two_parts"])
def test_schur_apply_is_the_eliminated_full_apply(name):
    """(1 - k D) [x_e; k D_oe x_e] has S x_e on the even rows and 0 on the odd ones"""
    c, p = ec.case(name), ec.case_plan(name)
    k = 0.11 + 0.02j
    xe = ec.rhs(p.even.size, 3)
    x = ec.reconstruct(p, k, np.zeros(c.n, ec.c128), xe)
    y = ec.dirac_apply(c, k, x)
    s = ec.schur_apply(p, k, xe)
    assert np.abs(y[p.even] - s).max() <= 1e-13 * np.abs(s).max()
    assert np.abs(y[p.odd]).max() <= 1e-13 * np.abs(s).max()


@pytest.fixture(scope="module")
def sample_solves():
    c, p = ec.case("sample"), ec.case_plan("sample")
    b = ec.rhs(c.n)
    out = {}
    for k in (0.15, 0.18):
        bhat = ec.prepare(p, k, b)
        xe, hist, it, conv = ec.gcr(lambda v: ec.schur_apply(p, k, v), bhat, 5, TOL, 4000)
        xf, _, itf, convf = ec.gcr(lambda v: ec.dirac_apply(c, k, v), b, 5, TOL, 4000)
        out[k] = dict(b=b, bhat=bhat, x=ec.reconstruct(p, k, b, xe), hist=hist, it=it, conv=conv, xf=xf, itf=itf, convf=convf)
    return out


@pytest.mark.parametrize("k", [0.15, 0.18])
def test_reconstructed_residual_is_the_mapped_history_entry(sample_solves, k):
    c, p, s = ec.case("sample"), ec.case_plan("sample"), sample_solves[k]
    assert s["conv"]
    r = ec.dirac_apply(c, k, s["x"]) - s["b"]
    true = np.linalg.norm(r) / np.linalg.norm(s["b"])
    mapped = s["hist"][-1] * np.linalg.norm(s["bhat"]) / np.linalg.norm(s["b"])
    assert abs(true / mapped - 1.0) <= 1e-6, (true, mapped)
    assert np.linalg.norm(r[p.odd]) / np.linalg.norm(s["b"]) <= 1e-13
    assert np.linalg.norm(s["x"] - s["xf"]) / np.linalg.norm(s["xf"]) <= 10 * TOL


@pytest.mark.parametrize("k", [0.15, 0.18])
def test_schur_solve_takes_fewer_steps(sample_solves, k):
    s = sample_solves[k]
    assert s["conv"] and s["convf"] and s["it"] < s["itf"], (s["it"], s["itf"])
