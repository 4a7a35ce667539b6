"""Premises of the even-odd low-precision GCR's cases (tests/gcr32_eo_cases.py), on the CPU and the numpy model alone: the fp32 Schur
model and the same algorithm in fp64 take equal outer and equal total inner step counts on every solvable case and inner setting (a
case where they do not would go into gcr32_eo_cases.SENSITIVE with both counts, after 1e-7 noise on the fp64 inner solve is shown to
move its count too); the mixed solves end at a true Schur residual <= 1e-10 (1 + 1e-3); the Schur complement written out as a CSR
matrix — what the outer model runs on — is the two-stage fp64 apply; the model's counts are those the issue was written with; and the
three host mutants — 1 / a_o left out of stage 1, c in place of c^2, the tail folded into the first accumulator — each fail Rule A's
comparison on at least one case."""
import json
import os

import numpy as np
import pytest

from tests import evenodd_diag_cases as dc
from tests import gcr32_cases as g
from tests import gcr32_eo_cases as e

KEYS = [(name, k, inner) for name, k in e.all_cases() for inner in e.inner_settings(name, k) if inner[2] > 0.]


def key_id(key):
    return "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1])


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64).reshape(-1, 2)


def test_values_and_right_hand_sides_are_not_floats():
    for name, k in e.all_cases():
        c = e.case(name, k)
        if c.form != "matrix":
            assert (c.val.real.astype(np.float32).astype(np.float64) != c.val.real).mean() > 0.9
        b = e.rhs(c.n)
        assert (b.real.astype(np.float32).astype(np.float64) != b.real).mean() > 0.9


@pytest.mark.parametrize("name,k", e.all_cases())
def test_the_written_out_schur_complement_is_the_two_stage_apply(name, k):
    c = e.case(name, k)
    p, co = e.dplan(c)
    x = e.rhs(p.even.size, 21)
    y = dc.schur_apply(p, co, x)
    ys, mag = g.apply_f64(e.schur_csr(name, c.k), x)
    assert np.abs(ys - y).max() <= 1e-12 * max(1., np.abs(mag).max())
    # ... and the fp32 model is the fp64 one to float's rounding
    y32 = e.EoModel(c).apply_c128(x)
    assert np.linalg.norm(y32 - y) <= 1e-5 * np.linalg.norm(y)


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_fp32_takes_the_step_counts_of_fp64(key):
    o32, o64 = e.mixed(*key, "f32"), e.mixed(*key, "f64")
    print(key_id(key), "fp32 %d / %d, fp64 %d / %d" % (o32.n_iter, o32.inner_total, o64.n_iter, o64.inner_total))
    assert o32.converged and o64.converged
    assert o32.true_res <= 1e-10 * (1 + 1e-3) and o64.true_res <= 1e-10 * (1 + 1e-3)
    if key in e.SENSITIVE:
        assert ((o32.n_iter, o32.inner_total), (o64.n_iter, o64.inner_total)) == e.SENSITIVE[key]
        noisy = e.mixed(*key, "f64", 1e-7)
        assert (noisy.n_iter, noisy.inner_total) != (o64.n_iter, o64.inner_total)
    else:
        assert (o32.n_iter, o32.inner_total) == (o64.n_iter, o64.inner_total)


def test_the_sample_has_the_counts_the_feature_was_proposed_with():
    """outer / inner Schur steps of the 3072-row sample: 22 / 87 and 8 / 56 at k = 0.15, 22 / 174 and 11 / 173 at k = 0.18"""
    want = {(0.15, e.INNER[0]): (22, 87), (0.15, e.INNER[1]): (8, 56), (0.18, e.INNER[0]): (22, 174), (0.18, e.INNER[1]): (11, 173)}
    for (k, inner), counts in want.items():
        o = e.mixed("sample", k, inner, "f32")
        assert (o.n_iter, o.inner_total) == counts, (k, inner)


def test_the_two_restart_setting_crosses_two_boundaries():
    r, m, tol = e.INNER_TWO_RESTARTS
    assert tol == 0. and m > 2 * r and e.INNER_TWO_RESTARTS in e.inner_settings("sample", 0.15)
    c = e.case("sample", 0.15)
    assert g.inner_solve(e.EoModel(c), e.rhs(e.plan_of("sample").ne), r, m, tol).n_iter == m


def rule_a_catches(name, **mutant):
    c = e.case(name)
    x = e.rhs(e.plan_of(name).ne, 21)
    good, bad = e.EoModel(c).apply_c128(x), e.EoModel(c, **mutant).apply_c128(x)
    return np.nonzero((bits(good) != bits(bad)).any(axis=1))[0]


def test_the_mutant_without_the_inverse_diagonal_is_caught_by_rule_a():
    for name in ("d_open4d", "d_scalar", "sample_twisted", "box_small", "box_many"):
        assert rule_a_catches(name, no_inv=True).size > 0, name
    assert rule_a_catches("sample", no_inv=True).size == 0          # nothing stored on the diagonal: the mutant is the model


def test_the_mutant_with_c_for_c2_is_caught_by_rule_a():
    for name in ("chain", "two_parts", "sample", "d_open4d", "d_scalar", "sample_twisted", "bip_long"):
        assert rule_a_catches(name, c_for_c2=True).size > 0, name
    # matrix form: c = -1 and c^2 = 1 differ in sign
    assert rule_a_catches("box_small", c_for_c2=True).size > 0


def test_the_mutant_that_folds_the_tail_is_caught_by_rule_a():
    for name in ("bip_long", "d_open4d"):
        p = e.plan_of(name)
        assert p.hplans[0].tail_rows.size and p.hplans[1].tail_rows.size
        assert rule_a_catches(name, fold_tail=True).size > 0, name
    # stage 2 alone: the rows that differ when only H_eo's tail is folded are H_eo's tail rows
    c = e.case("bip_long")
    x = e.rhs(e.plan_of("bip_long").ne, 21)
    good, bad = e.EoModel(c), e.EoModel(c)
    bad.h[0] = e.HalfModel(bad.p.halves[0], bad.p.hplans[0], e.f32, fold_tail=True)
    rows = np.nonzero((bits(good.apply_c128(x)) != bits(bad.apply_c128(x))).any(axis=1))[0]
    assert rows.size > 0 and np.isin(rows, bad.p.hplans[0].tail_rows).all()
    assert rule_a_catches("sample", fold_tail=True).size == 0        # no tail: the mutant is the model


def test_the_refusal_cases_are_refused_by_the_model_and_the_others_are_not():
    for name in e.REJECTED:
        c, row, word = e.rejected(name)
        assert e.refusal(c) == (row, word), name
    for name, k in e.all_cases():
        assert e.refusal(e.case(name, k)) is None, name


def test_the_recorded_device_figures_keep_rules_b_and_c():
    """tests/golden/observed_gcr32_eo.json, written by tests/test_gpu_gcr32_eo.py on an MI355X: every inner solve's error against the
    fp64 algorithm is within 4 x the model's, and every mixed solve took the model's outer count"""
    obs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observed_gcr32_eo.json")))
    all_keys = [(name, k, inner) for name, k in e.all_cases() for inner in e.inner_settings(name, k)]
    assert sorted(obs["rule_b"]) == sorted(key_id(k) for k in all_keys)
    for name, r in obs["rule_b"].items():
        assert r["ratio"] <= 4. and r["n_iter"] >= 1, (name, r)
    assert sorted(obs["rule_c"]) == sorted(key_id(k) for k in KEYS)
    for key in KEYS:
        r = obs["rule_c"][key_id(key)]
        assert r["true_schur_residual"] <= 1e-10 * (1 + 1e-3), (key, r)
        if key not in e.SENSITIVE:
            assert r["outer"] == r["model_outer"] == e.mixed(*key, "f32").n_iter, (key, r)
