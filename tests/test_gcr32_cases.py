"""Premises of the low-precision GCR's cases (tests/gcr32_cases.py), on the CPU and the numpy model alone: each case has what it claims;
the fp32 apply differs from the fp64 apply by no more than (row length + 2) 2^-24 sum |a_ij| |x_j| per row; the fp32 model and the same
algorithm in fp64 take equal outer and equal total inner step counts; no stopping test, inner or outer, comes within 1e-3 relative
of its threshold, so that no step count hangs on a tie; and the two host mutants — a tail folded into the first accumulator, an
alpha rounded before its division — are caught by the checks the GPU test uses (Rule A's bits, the one-step solve's bits).

The outer model is the library's fp64 GCR, which keeps the reference's conjugation of alpha and beta (csrc/gcr.hip); the counts are
therefore those of mgcr_gcr_solve, not of a minimal-residual outer iteration.
The mixed solves of the real operators (b, c) take a real right-hand side (gcr32_cases.rhs_mixed): with complex data on a real
symmetric operator that conjugation makes the outer iteration amplify ANY 1e-7 perturbation of the preconditioner's output into a
different step count (fp32 7 / 78 against 5 / 57 on the 9 x 7 x 5 box at 16 steps, tol 0.01; an fp64 inner solve with 1e-7 noise
6 / 68; 26 / 204 against 23 / 180 on the 33 x 31 x 31 box at 8 steps, tol 0.1), which says nothing about fp32."""
import numpy as np
import pytest

from tests import gcr32_cases as g

KEYS = [(name, k, inner) for name, k in g.all_cases() for inner in g.inner_settings(name)]


def key_id(key):
    return "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1])


def test_each_case_has_what_it_claims():
    plans = {name: g.plan(g.case(name)) for name in g.CASES}
    assert g.case("a").n == 3072 and not plans["a"].real
    assert g.case("b").n == 315 < g.TILE and plans["b"].real and plans["b"].W == 7            # odd n, less than one workgroup, real slab
    assert g.case("c").n == 31713 and g.case("c").n % 2 == 1 and g.case("c").n % g.TILE != 0 and g.case("c").n > 30 * g.TILE and plans["c"].real
    d = g.case("d")
    assert d.n == 1152 and (np.diff(d.rowptr) == 24).all() and plans["d"].W == 24 and not plans["d"].real and plans["d"].tail_rows.size == 0
    e, pe = g.case("e"), plans["e"]
    lens = np.diff(e.rowptr)
    assert e.n == 3001 and pe.tail_rows.size > 0 and (lens[pe.tail_rows] > pe.W).all() and lens.min() >= 1 and lens.max() >= 100
    assert (lens > 2 * pe.W).sum() == 3 and np.unique(lens).size >= 12                          # the three long rows; a spread of lengths
    assert pe.tile_tail[0] == 0 and pe.tile_tail[-1] == pe.tail_rows.size and (np.diff(pe.tile_tail) > 0).all()   # every tile has tail rows
    assert g.case("f").n == 45 < 64
    for name in g.CASES:                                                                        # values that are not floats
        c = g.case(name)
        if name not in ("b", "c"):
            assert (c.val.real.astype(np.float32).astype(np.float64) != c.val.real).mean() > 0.9
        b = g.rhs(c.n)
        assert (b.real.astype(np.float32).astype(np.float64) != b.real).mean() > 0.9
        for k in g.CASES[name]:
            assert k is None or float(np.float32(k)) != k
    assert g.bad_row(g.case("g", None)) == g.G_ROW and g.bad_row(g.case("d")) == -1


def test_case_e_needs_twenty_plain_steps():
    c = g.case("e")
    plain = g.outer_solve(c, g.rhs(c.n), None, **g.OUTER)
    assert plain.converged and plain.n_iter >= 20, plain.n_iter


@pytest.mark.parametrize("name,k", g.all_cases())
def test_the_fp32_apply_is_within_its_rounding_bound(name, k):
    c = g.case(name, k)
    x = g.rhs(c.n, 21)
    y64, mag = g.apply_f64(c, x)
    y32 = g.Model(c).apply_c128(x)
    lens = np.diff(c.rowptr)
    if k is not None:                     # x - k s: the row sum is scaled by |k| and x joins the sum
        mag = abs(k) * mag + np.abs(x)
    assert (np.abs(y32 - y64) <= (lens + 2) * 2. ** -24 * mag * np.sqrt(2)).all()               # (sqrt 2: real and imaginary parts each keep the bound)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_fp32_takes_the_step_counts_of_fp64(key):
    o32, o64 = g.mixed(*key, "f32"), g.mixed(*key, "f64")
    print(key_id(key), "fp32 %d / %d, fp64 %d / %d" % (o32.n_iter, o32.inner_total, o64.n_iter, o64.inner_total))
    assert o32.converged and o64.converged and o32.true_res <= 1e-10 * (1 + 1e-3)
    assert (o32.n_iter, o32.inner_total) == (o64.n_iter, o64.inner_total)


@pytest.mark.parametrize("key", g.COMPLEX_ON_REAL, ids=key_id)
def test_complex_data_on_the_real_operators_and_the_known_exceptions(key):
    """The same premise with the complex right-hand side on the real operators: two of the four take fp64's counts, the other two are
    the known exceptions (gcr32_cases.SENSITIVE), held to the counts they were found with"""
    o32, o64 = g.mixed(*key, "f32", True), g.mixed(*key, "f64", True)
    print(key_id(key), "fp32 %d / %d, fp64 %d / %d" % (o32.n_iter, o32.inner_total, o64.n_iter, o64.inner_total))
    assert o32.converged and o64.converged and o32.true_res <= 1e-10 * (1 + 1e-3)
    if key in g.SENSITIVE:
        assert ((o32.n_iter, o32.inner_total), (o64.n_iter, o64.inner_total)) == g.SENSITIVE[key]
    else:
        assert (o32.n_iter, o32.inner_total) == (o64.n_iter, o64.inner_total)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_no_stopping_test_is_a_near_tie(key):
    for dt in ("f32", "f64"):
        o = g.mixed(*key, dt)
        for m in (o.margins, o.inner_margins):
            assert len(m) == 0 or np.abs(np.array(m) - 1.).min() >= 1e-3      # (tol 0: the inner solve has no stopping test)


def test_the_two_restart_setting_crosses_two_boundaries_at_every_k():
    r, m, tol = g.INNER_TWO_RESTARTS
    assert tol == 0. and m > 2 * r
    for k in g.CASES["a"]:
        c = g.case("a", k)
        assert g.inner_solve(g.Model(c), g.rhs(c.n), r, m, tol).n_iter == m


def test_the_recorded_device_figures_keep_rule_b():
    """tests/golden/observed_gcr32.json, written by tests/test_gpu_gcr32.py on an MI355X: every inner solve's error against the
    fp64 algorithm is within 4 x the model's (in fact equal: the device's y has the model's bits on every case)"""
    import json
    import os
    obs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observed_gcr32.json")))
    assert sorted(obs["rule_b"]) == sorted(key_id(k) for k in KEYS)
    for name, r in obs["rule_b"].items():
        assert r["ratio"] <= 4. and r["n_iter"] >= 1, (name, r)


def test_the_mutant_that_folds_the_tail_is_caught_by_rule_a():
    c = g.case("e")
    x = g.rhs(c.n, 21)
    good, bad = g.Model(c).apply_c128(x), g.Model(c, fold_tail=True).apply_c128(x)
    rows = np.nonzero(good.view(np.uint64).reshape(-1, 2) != bad.view(np.uint64).reshape(-1, 2))[0]
    assert rows.size > 0 and np.isin(rows, g.plan(c).tail_rows).all()
    c = g.case("d")                       # no tail: the mutant is the model
    assert np.array_equal(g.Model(c).apply_c128(x[:c.n]).view(np.uint64), g.Model(c, fold_tail=True).apply_c128(x[:c.n]).view(np.uint64))


def test_the_mutant_that_rounds_alpha_early_is_caught_by_the_one_step_bits():
    caught = 0
    for name, k in g.all_cases():
        c = g.case(name, k)
        f = g.rhs(c.n)
        m = g.Model(c)
        good, bad = g.inner_solve(m, f, 1, 1, 0.), g.inner_solve(m, f, 1, 1, 0., alpha_mutant=True)
        caught += not np.array_equal(good.y.view(np.uint64), bad.y.view(np.uint64))
    assert caught >= 3, caught
