"""Premises of the even-odd Schur solve with a dense block per site, on the numpy model of tests/evenodd_block_cases.py alone (CPU):
the model's Schur apply, prepare and reconstruct agree with a dense solve of A; every solve case converges at tol 1e-8 within the
step cap, in fewer steps than the full system, with a true full residual <= tol |bhat_e| (1 + 1e-3); the pivot case really swaps;
the refusal cases fail where they say.  The accuracy of the elimination is judged against LAPACK, not against itself: for every
block, rho = max(|BX - I|_inf, |XB - I|_inf) / (u |B|_inf |X|_inf) in extended precision, for the model's X and for np.linalg.inv;
per case max rho_model <= 2 max(max rho_LAPACK, 1) (Gauss-Jordan is not LU: the factor 2).  Both maxima per case are recorded in
tests/golden/observed_evenodd_block.json."""
import json
import os

import numpy as np
import pytest

from tests import evenodd_cases as ec
from tests import evenodd_block_cases as bc

OBSERVED = os.path.join(ec.GOLDEN, "observed_evenodd_block.json")
U = 2.0 ** -53


TOO_BIG_FOR_DENSE = ("grid2d_varied_b3", "w7_b16")      # 196 608 and 16 384 rows


@pytest.mark.parametrize("name", [n for n in bc.ALL if n not in TOO_BIG_FOR_DENSE])
def test_model_agrees_with_a_dense_solve(name):
    m = bc.model(name)
    c, p = m.bc, m.plan
    A = bc.dense(c)
    e, o = p.even, p.odd
    Aoo_inv = np.linalg.inv(A[np.ix_(o, o)])
    S = A[np.ix_(e, e)] - A[np.ix_(e, o)] @ Aoo_inv @ A[np.ix_(o, e)]
    x = ec.rhs(e.size, 3)
    want = S @ x
    scale = np.linalg.cond(A[np.ix_(o, o)])
    assert np.abs(bc.schur_apply(m, x) - want).max() <= 1e-13 * scale * np.abs(want).max()
    b = ec.rhs(c.n, 4)
    want = b[e] - A[np.ix_(e, o)] @ (Aoo_inv @ b[o])
    assert np.abs(bc.prepare(m, b) - want).max() <= 1e-13 * scale * np.abs(want).max()
    if name == "singular_even":
        return                      # (S is still regular here, but nothing below is about the even block)
    xe = np.linalg.solve(S, bc.prepare(m, b))
    xf = bc.reconstruct(m, b, xe)
    assert np.linalg.norm(A @ xf - b) <= 1e-13 * scale * np.linalg.cond(S) * np.linalg.norm(b)


def test_the_dense_skip_leaves_only_the_widest_case():
    big = [n for n in bc.ALL if bc.case(n).n > 4000]
    assert sorted(big) == sorted(TOO_BIG_FOR_DENSE)


def test_schur_identity_on_the_wide_case_through_the_full_operator():
    """w7_b16 (16 384 rows): S x_e against the full operator applied to the reconstructed vector — A [x_e; x_o] = [S x_e; 0] when
    x_o = B_o^-1 c H_oe x_e"""
    m = bc.model("w7_b16")
    p = m.plan
    xe = ec.rhs(p.even.size, 5)
    xf = bc.reconstruct(m, np.zeros(p.n, ec.c128), xe)
    y = bc.full_apply(m.bc, xf)
    want = bc.schur_apply(m, xe)
    assert np.abs(y[p.even] - want).max() <= 1e-11 * np.abs(want).max()
    assert np.abs(y[p.odd]).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("name", bc.SOLVABLE)
def test_solve_cases_converge_in_fewer_steps_than_the_full_system(name):
    m = bc.model(name)
    c, p = m.bc, m.plan
    b = ec.rhs(c.n)
    bhat = bc.prepare(m, b)
    xe, hist, it, conv = ec.gcr(lambda v: bc.schur_apply(m, v), bhat, 5, bc.TOL, bc.STEP_CAP)
    assert conv and it < bc.STEP_CAP, (it, hist[-1])
    xf = bc.reconstruct(m, b, xe)
    true = np.linalg.norm(bc.full_apply(c, xf) - b)
    _, fhist, fit, fconv = ec.gcr(lambda v: bc.full_apply(c, v), b, 5, bc.TOL, 4 * bc.STEP_CAP)
    print("%s: Schur %d steps, full %d steps (converged %s), true residual %.3e |bhat_e|" % (name, it, fit, fconv,
                                                                                          true / np.linalg.norm(bhat)))
    assert true <= bc.TOL * np.linalg.norm(bhat) * (1 + 1e-3)
    assert it < fit


def test_the_pivot_case_really_swaps():
    m = bc.model("pivot_swap")
    _, so = bc.site_lists(m.plan, m.bc.bs)
    at = int(np.nonzero(so == 1)[0][0])
    assert m.co.B[1][0, 0] == 0 and m.swaps[at] >= 1 and (m.failed < 0).all()
    assert np.abs(m.invBo[at] @ m.co.B[1] - np.eye(3)).max() <= 1e-14


def test_special_blocks_are_what_the_cases_say():
    m = bc.model("cond1e8")
    assert 3e7 <= np.linalg.cond(m.co.B[3]) <= 3e8 and m.plan.parity[3 * 4] == 1
    m = bc.model("singular_even")
    assert np.linalg.matrix_rank(m.co.B[2]) == 1 and m.plan.parity[2 * 2] == 0 and (m.failed < 0).all()
    m = bc.model("no_insite")
    assert np.array_equal(m.co.B[2], np.eye(2)) and np.array_equal(m.co.B[3], np.eye(2))
    assert bc.strip("dup_insite")[2] == 6 * 4 + 3
    p = bc.case_plan("open4d_b5")
    assert p.even.size != p.odd.size and min(p.even.size, p.odd.size) // 5 > 12
    assert bc.case("chain_b2").n == 12 and bc.case("sample_h10").n == 3072 and bc.case("w7_b16").bs == 16


def test_refusal_cases_fail_where_they_say():
    c, site, row = bc.rejected("singular_odd")
    m = bc.model_of(c, bc.plan_of(c))
    _, so = bc.site_lists(m.plan, c.bs)
    s, p = bc.first_failure(m.failed)
    assert (int(so[s]), int(so[s]) * c.bs + p) == (site, row)
    good, k_bad, site, row = bc.rejected("set_k_singular")
    m = bc.model_of(good, bc.plan_of(good))
    assert bc.first_failure(m.failed) is None
    m = bc.model_of(bc.with_k(good, k_bad), bc.plan_of(good))
    _, so = bc.site_lists(m.plan, good.bs)
    s, p = bc.first_failure(m.failed)
    assert (int(so[s]), int(so[s]) * good.bs + p) == (site, row)
    c, entry = bc.rejected("triangle")
    assert entry is not None and entry[0] // c.bs != entry[1] // c.bs
    assert bc.rejected("not_whole").n % bc.rejected("not_whole").bs != 0
    _, par, entry = bc.rejected("flipped")
    assert entry is not None and par[entry[0]] == par[entry[1]]


# ---- the elimination against LAPACK -------------------------------------------------------------------------------------------------
def rho(B, X):
    """max(|BX - I|_inf, |XB - I|_inf) / (u |B|_inf |X|_inf) per block, in extended precision"""
    Bl, Xl = B.astype(np.clongdouble), X.astype(np.clongdouble)
    eye = np.eye(B.shape[-1], dtype=np.clongdouble)
    norm = lambda M: np.abs(M).sum(axis=2).max(axis=1)           # noqa: E731
    res = np.maximum(norm(np.einsum("sij,sjk->sik", Bl, Xl) - eye), norm(np.einsum("sij,sjk->sik", Xl, Bl) - eye))
    return (res / (np.longdouble(U) * norm(Bl) * norm(Xl))).astype(np.float64)


def rho_maxima(name):
    m = bc.model(name)
    _, so = bc.site_lists(m.plan, m.bc.bs)
    B = m.co.B[so]
    assert (m.failed < 0).all()
    return float(rho(B, m.invBo).max()), float(rho(B, np.linalg.inv(B)).max())


@pytest.mark.parametrize("name", bc.ALL)
def test_elimination_is_as_accurate_as_lapack(name):
    mine, lapack = rho_maxima(name)
    print("%s: max rho of the model %.3f, of LAPACK %.3f" % (name, mine, lapack))
    assert mine <= 2 * max(lapack, 1.0), (mine, lapack)
    seen = json.load(open(OBSERVED))
    assert name in seen and set(seen[name]) == {"rho_model", "rho_lapack"}
    assert seen[name]["rho_model"] <= 2 * max(seen[name]["rho_lapack"], 1.0)
    assert abs(seen[name]["rho_model"] - mine) <= 0.05 * max(mine, 1.0)       # the recorded figure is this model's


if __name__ == "__main__":       # python -m tests.test_evenodd_block_cases: rewrite the recorded maxima
    out = {}
    for case_name in bc.ALL:
        a, b = rho_maxima(case_name)
        out[case_name] = {"rho_model": round(a, 4), "rho_lapack": round(b, 4)}
    with open(OBSERVED, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))
