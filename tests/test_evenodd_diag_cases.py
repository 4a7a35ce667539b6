"""The premises of the even-odd Schur solve with a site diagonal, on the numpy model of tests/evenodd_diag_cases.py alone (no GPU, no
library): per solvable case, GCR(5) at tol 1e-10 from x0 = 0 converges on the Schur system in fewer steps than on the full one, the
full system's true residual is the mapped last history entry, and the odd half of the residual is rounding.  These are the
conditions tests/test_gpu_evenodd_diag.py asks of the device.  Plus the shape of the case table itself."""
import numpy as np
import pytest

from tests import evenodd_cases as ec
from tests import evenodd_diag_cases as dc

TOL = 1e-10


@pytest.mark.parametrize("name", dc.SOLVABLE)
def test_schur_solve_premises_on_the_model(name):
    d, p, co = dc.model(name)
    b = ec.rhs(d.n)
    bn = np.linalg.norm(b)
    _, _, it_full, conv_full = ec.gcr(lambda v: dc.full_apply(d, v), b, 5, TOL, 4000)
    bhat = dc.prepare(p, co, b)
    xe, hist, it_schur, conv_schur = ec.gcr(lambda v: dc.schur_apply(p, co, v), bhat, 5, TOL, 4000)
    x = dc.reconstruct(p, co, b, xe)
    r = dc.full_apply(d, x) - b
    true, mapped, odd = np.linalg.norm(r) / bn, hist[-1] * np.linalg.norm(bhat) / bn, np.linalg.norm(r[p.odd]) / bn
    print("%s: full %d steps, Schur %d; true %.6e, mapped %.6e, |difference| %.3e, odd half %.3e" % (name, it_full, it_schur, true, mapped,
                                                                                                    abs(true - mapped), odd))
    assert conv_full and conv_schur
    assert it_schur < it_full
    assert abs(true - mapped) <= 1e-14
    assert odd <= 1e-14


def test_the_schur_model_is_the_full_operator_eliminated():
    """S x_e = (A x)_e for x = (x_e, x_o) with x_o chosen so that (A x)_o = 0: the elimination the device performs"""
    for name in ("d_open4d", "poisson_box", "sample_twisted"):
        d, p, co = dc.model(name)
        xe = ec.rhs(p.even.size, 7)
        x = dc.reconstruct(p, co, np.zeros(d.n, ec.c128), xe)
        y = dc.full_apply(d, x)
        s = dc.schur_apply(p, co, xe)
        assert np.abs(y[p.odd]).max() <= 1e-13 * np.abs(s).max()
        assert np.abs(y[p.even] - s).max() <= 1e-13 * np.abs(s).max()


def test_case_table():
    assert set(dc.FUSED_FORMS) <= set(dc.FUSED) <= set(dc.ALL) and set(dc.SOLVABLE) <= set(dc.ALL)
    assert sorted(n[2:] for n in dc.DIRAC_ALL) == sorted(ec.ALL)
    for name in dc.ALL:
        d, p, co = dc.model(name)
        hop, diag, n_diag = dc.strip(name)
        base = {"poisson_box": None, "chain_zero_even": "chain", "dup_diag": "chain", "sample_twisted": "sample"}.get(
            name, name[2:] if name in dc.DIRAC_ALL else name[:-2])
        if base is not None:        # the halves are the hopping case's halves: every storage form the existing tests pin is reached again
            c = ec.case(base)
            assert np.array_equal(hop.rowptr, c.rowptr) and np.array_equal(hop.col, c.col) and np.array_equal(hop.val, c.val)
        assert np.isfinite(dc.einv(co.a[p.odd])).all() and (dc.einv(co.a[p.odd]) != 0).all()
    assert np.abs(dc.strip("d_open4d")[1].real).max() <= 1 and np.abs(dc.strip("d_open4d")[1].imag).max() <= 1
    # a_e exactly zero on one even row; two stored diagonal entries added in stored order; an explicit zero is a diagonal entry
    d, p, co = dc.model("chain_zero_even")
    assert p.parity[4] == 0 and co.a[4] == 0 and np.count_nonzero(co.a == 0) == 1
    assert dc.strip("dup_diag")[2] == 3 and dc.strip("dup_diag")[1][3] == (0.25 - 0.5j) + (1e-3 + 2.0j) and dc.strip("dup_diag")[1][6] == 0
    bad, good, k_bad, row = dc.rejected("singular_odd")
    hop, diag, _ = dc.strip_case(bad)
    assert ec.plan(hop).parity[row] == 1 and dc.coefficients(bad, diag).a[row] == 0
    assert dc.coefficients(good, diag).a[row] == 0.5 and k_bad == bad.k
    assert dc.case("poisson_box").n == 120 and dc.case_plan("poisson_box").even.size < 64
