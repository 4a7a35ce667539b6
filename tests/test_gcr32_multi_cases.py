"""Premises of the batched mixed solve's tests, checked on the numpy model alone (tests/gcr32_multi_cases.py); no GPU needed.

(a) Every Rule M2 case and inner setting converges to 1e-10 within the tests' max_outer = 40, and the fp32 model takes the fp64
    model's outer and inner step counts; no outer or inner stopping test sits at its threshold, so a count does not hang on the order
    of an fp64 sum (the only difference between the device and the model).
(b) The ragged block of Rule M1 is ragged: its columns' inner step counts take at least three distinct values, 0 (the zero column)
    and max_iter (a column that misses its tolerance) among them; the duplicate column repeats column 0.
(c) The Rule M2 blocks are ragged through x0: outer counts 0 (the converged x, the zero column), the full count and the full count
    less 3 all occur, and the model continued from its x after 3 steps takes exactly the remaining steps."""
import numpy as np
import pytest

from tests import gcr32_cases as g
from tests import gcr32_multi_cases as mc

KEYS = [(name, k, inner) for name, k in mc.M2_CASES for inner in g.INNER]


def key_id(key):
    return "%s-k%s-r%d-m%d" % (key[0], key[1], key[2][0], key[2][1])


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_premise_a_the_model_converges_and_fp32_takes_fp64s_counts(key):
    name, k, inner = key
    s32, s64 = mc.solved(name, k, inner, "f32"), mc.solved(name, k, inner, "f64")
    print(key_id(key), "outer", s32.n_outer, "inner", s32.inner_total, "last |r| / |b| %.2e" % s32.hist[-1])
    assert s32.converged and s64.converged and s32.n_outer <= mc.MAX_OUTER
    assert s32.hist[-1] <= mc.TOL
    assert s32.n_outer == s64.n_outer and s32.inner_iters == s64.inner_iters
    # no test at its threshold: the outer residuals are a factor 1.1 away from tol, the inner ones 0.1 % away from theirs
    assert all(abs(np.log(h / mc.TOL)) > np.log(1.1) for h in s32.hist)
    assert all(abs(np.log(x)) > 1e-3 for x in s32.inner_margins if x > 0)


def test_premise_a_the_counts_of_the_issue():
    """(8, 8, 0.1): 8 - 10 outer steps, 20 on the sample at 0.18; (16, 16, 0.01): 5 and 10; 24 - 160 inner steps in all"""
    for name, k in mc.M2_CASES:
        hard = (name, k) == ("a", 0.18)
        s8, s16 = mc.solved(name, k, g.INNER[0]), mc.solved(name, k, g.INNER[1])
        assert s8.n_outer == 20 if hard else 8 <= s8.n_outer <= 10, (name, k, s8.n_outer)
        assert s16.n_outer == (10 if hard else 5), (name, k, s16.n_outer)
        assert 24 <= s8.inner_total <= 160 and 24 <= s16.inner_total <= 160


def test_premise_b_the_ragged_block_is_ragged():
    F, iters, rels = mc.ragged_block()
    _, _, (restart, max_iter, tol) = mc.RAGGED
    print("inner steps per column", iters, "|r| / |f|", ["%.3f" % r for r in rels])
    assert len(set(iters)) >= 3 and 0 in iters and max_iter in iters
    zero = len(mc.RAGGED_SEEDS)
    assert not F[zero].any() and iters[zero] == 0
    assert np.array_equal(F[zero + 1], F[0]) and iters[zero + 1] == iters[0]
    assert any(i == max_iter and r > tol * 1.001 for i, r in zip(iters, rels))          # a column that misses its tolerance
    assert any(0 < i < max_iter and r <= tol for i, r in zip(iters, rels))              # and one that meets it early
    assert 2 <= F.shape[0] <= 16


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_premise_c_the_x0_blocks_take_different_outer_counts(key):
    name, k, inner = key
    c = g.case(name, k)
    for width in (3, 8):
        blk = mc.m2_block(name, k, inner, width)
        full = mc.solved(name, k, inner, "f32", mc.M2_KINDS[width][0][1]).n_outer
        assert 0 in blk.n_outer and len(set(blk.n_outer)) >= 3, blk.n_outer
        assert min(n for n in blk.n_outer if n) >= 1 and max(blk.n_outer) <= mc.MAX_OUTER
        assert full > 3
    # the model continued from its x after 3 steps takes the remaining steps, and none from its converged x
    s = mc.solved(name, k, inner)
    m = mc.model(name, k, "f32")
    assert mc.defect_solve(c, m, g.rhs(c.n), inner, x0=s.xs[3]).n_outer == s.n_outer - 3
    assert mc.defect_solve(c, m, g.rhs(c.n), inner, x0=s.x).n_outer == 0
