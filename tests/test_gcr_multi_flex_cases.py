"""The premises of the flexible batched GCR's GPU tests, checked on the numpy model alone (tests/gcr_multi_flex_cases.py), so that
the blocks tests/test_gpu_gcr_multi_flex.py runs exercise what they claim:
  (i)   in the restart-5 block a column stops inside a cycle with x updates pending while another runs at least a whole cycle more
        — the case an exit kernel that is not masked corrupts;
  (ii)  in the restart-3 block columns stop on a step that closes a cycle;
  (iii) there are blocks for restart 1 (every step closes), restart 5 and max_iter < restart (the shortened storage);
  (iv)  the max_iter block runs into its limit with a column unconverged beside converged ones;
and the blocks hold a zero column, a duplicate column and every width's group shape."""
import numpy as np

from tests import gcr32_cases as g
from tests import gcr_multi_flex_cases as fc

NAME, K, INNER = fc.PREMISE
COLS = fc.COLUMNS[:6]          # the premises rest on the first columns: every width from 5 on contains them


def counts(outer, cols=COLS):
    return fc.model_counts(NAME, K, INNER, outer, cols)


def decided(margins):
    """the stop is not a near miss: the last test that failed and the one that passed are both 20 % away from the tolerance"""
    return margins[-1] < 0.8 and (len(margins) < 2 or margins[-2] > 1.2)


def test_the_blocks_hold_a_zero_column_a_duplicate_and_every_group_shape():
    assert fc.WIDTHS == (1, 3, 5, 16) and len(fc.COLUMNS) == 16
    assert fc.COLUMNS[2] == ("null", 0) and fc.COLUMNS[3] == fc.COLUMNS[0]
    c = g.case(NAME, K)
    blk = fc.make_block(NAME, K, fc.COLUMNS[:5])
    assert not blk.B[2].any() and not blk.X0[2].any() and np.array_equal(blk.B[3], blk.B[0])
    assert blk.X0[1].any() and blk.X0[4].any() and not blk.X0[0].any()                  # "mid" columns start from the model's x
    assert max(t for kind, _ in fc.COLUMNS if isinstance(kind, tuple) for t in [kind[1]]) <= fc.PLAIN_STEPS
    for j in (1, 4):                                                                    # ... which is nearer the solution than 0
        b = blk.B[j]
        assert np.linalg.norm(b - g.apply_f64(c, blk.X0[j])[0]) < 0.1 * np.linalg.norm(b)


def test_premise_i_a_column_stops_inside_a_cycle_while_another_runs_a_cycle_more():
    restart, max_iter, _ = fc.OUTER_5
    res = counts(fc.OUTER_5)
    its = [r[0] for r in res]
    print("restart 5: stop steps", its)
    assert all(r[1] for r in res)
    assert fc.pending_and_runner(its, restart, max_iter)
    # ... with a decided stop, and for more than one pair of columns
    early = [j for j, r in enumerate(res) if r[0] % restart != 0 and r[0] > 1 and max(its) - r[0] >= restart and decided(r[2])]
    assert early, its
    assert its[2] == 1 and its[3] == its[0]                                             # the zero column ends at its first test
    assert len(set(its)) >= 4


def test_premise_ii_columns_stop_on_a_closing_step():
    restart, max_iter, _ = fc.OUTER_3
    res = counts(fc.OUTER_3)
    its = [r[0] for r in res]
    print("restart 3: stop steps", its)
    closing = [j for j, r in enumerate(res) if r[0] % restart == 0 and r[0] < max_iter]
    assert len(closing) >= 2 and len({its[j] for j in closing}) >= 2, its              # at different steps, others running on
    assert max(its) > min(its[j] for j in closing)
    assert fc.pending_and_runner(its, restart, max_iter)                                # and premise (i) at this cycle length too


def test_premise_iii_restart_one_and_the_shortened_storage():
    res1 = counts(fc.OUTER_1, COLS[:5])
    its1 = [r[0] for r in res1]
    print("restart 1: stop steps", its1)
    assert all(r[1] for r in res1) and len(set(its1)) >= 3
    restart, max_iter, _ = fc.OUTER_SHORT
    assert max_iter < restart
    short = counts(fc.OUTER_SHORT, COLS)
    print("max_iter < restart: stop steps", [r[0] for r in short])
    assert [r[0] for r in short[:2]] == [max_iter, max_iter] and not short[0][1]        # runs into the limit inside its first cycle
    assert any(r[1] and r[0] > 1 for r in short)                                        # ... beside a column that converges there
    assert fc.OUTER_5[0] == 5 and fc.OUTER_LIMIT[0] == 5


def test_premise_iv_the_limit_block_leaves_a_column_unconverged():
    restart, max_iter, _ = fc.OUTER_LIMIT
    res = counts(fc.OUTER_LIMIT)
    its = [r[0] for r in res]
    print("max_iter 12: stop steps", its, [r[1] for r in res])
    assert not res[0][1] and its[0] == max_iter and res[0][2][-1] > 100.                # far from converged at the limit
    conv = [j for j, r in enumerate(res) if r[1] and 1 < r[0] < max_iter - 1]
    assert conv, its                                                                    # frozen columns beside it when the solve ends
