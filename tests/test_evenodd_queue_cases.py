"""The premises of the queued even-odd scan's GPU tests (tests/test_gpu_evenodd_queue.py), checked on the numpy model of
tests/evenodd_cases.py — no GPU needed.  For every ladder of tests/evenodd_queue_cases.py and every width strictly between 1 and the
number of systems, the schedule that follows from the model's iteration counts admits a system after step 0 beside a running column
and retires a column at a cycle boundary at which another goes on; the counts end in at least three different restart cycles, which
leaves room for the device's counts (they differ: the model lacks the reference's conjugation).  And the queue
is worth having on the sample ladder: at widths 2 and 3 it takes fewer lockstep steps than waiting for each group of columns."""
import pytest

from tests import evenodd_multi_cases as emc
from tests import evenodd_queue_cases as eq
from tests import queue_cases as qc


@pytest.mark.parametrize("name", sorted(eq.LADDERS))
def test_the_schedule_refills_beside_running_columns(name):
    lad = eq.LADDERS[name]
    its = eq.model_stops(name)
    print(name, its)
    assert eq.cycles_spread(its, lad.restart) >= 3, its
    widths = eq.interior_widths(lad)
    assert widths, "a ladder needs a width at which a slot is refilled beside a running column"
    for w in widths:
        assert eq.premise(its, w, lad.restart) == (True, True), (w, its)


def test_the_premise_tells_schedules_apart():
    assert eq.premise([10, 10, 10, 10], 2, 5) == (False, False)        # both columns stop together: nothing runs beside a refill
    assert eq.premise([30, 8, 8], 2, 5) == (True, True)
    assert eq.premise([8, 30], 2, 5) == (False, True)                  # nothing waits when the short column retires
    assert eq.interior_widths(eq.LADDERS["sample"]) == [2, 3]


def test_the_sample_ladder_is_the_one_of_the_batched_scan():
    assert eq.model_stops("sample") == emc.LADDER_MODEL_STOPS
    for name in ("sample_longest_first", "sample_shuffled"):
        assert sorted(eq.model_stops(name)) == sorted(emc.LADDER_MODEL_STOPS)
    assert eq.model_stops("sample_longest_first")[0] == emc.LADDER_MAX_ITER


@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("name", ["sample", "sample_longest_first", "sample_shuffled"])
def test_the_queue_takes_fewer_steps_than_waiting_for_each_group(name, width):
    """Fewer wherever the longest value is not the last of the list (width 2: 200 against 315 longest first, 200 against 325
    shuffled).  In the GIVEN order the ladder ascends and its last value, the one that runs to the cap, is admitted last under
    either policy and ends the list alone: both take 260 steps at width 2 and 235 at width 3 — equal, never more."""
    lad = eq.LADDERS[name]
    its = eq.model_stops(name)
    queued, grouped = qc.lockstep_steps(its, width, lad.restart), qc.wait_for_group_steps(its, width, lad.restart)
    print(name, width, queued, grouped)
    if name == "sample":
        assert queued == grouped == {2: 260, 3: 235}[width]
    else:
        assert queued < grouped


def test_more_than_sixteen_systems_and_distinct_values():
    for name in ("scalar20", "chain20"):
        ks = eq.LADDERS[name].ks
        assert len(ks) == 20 > 16 and len(set(ks)) == 20 and sum(1 for k in ks if k.imag != 0) == 1
        k0 = emc.case_k(eq.LADDERS[name].case)
        assert abs(ks[0] - 0.3 * k0) < 1e-15 and abs(ks[-1] - k0) < 1e-15
    for name in ("long", "lanes", "grid2d_const", "scalar_ti", "two_parts"):
        assert len(eq.LADDERS[name].ks) >= 5 and eq.LADDERS[name].widths == (2,)
