"""The queued batched GCR (mgcr_gcr_solve_queue): a Python model of its schedule (csrc/queue_plan.h) and the hand-computed cases that
tests/test_queue_plan.py runs through the C++ schedule on the CPU and tests/test_gpu_queue.py through the solver on the GPU.

Model: a system admitted at step G that stops after `it` steps of its own ends at E = G + it; the host learns of it, and refills the
slot, at the next boundary of the restart cycle, ceil(E / restart) * restart; waiting systems are admitted first in, first out, the
lowest free slot first; the solve has launched as many lockstep steps as the largest such boundary.  Valid when max_iter and
check_every are multiples of restart (every poll and every last step then falls on a boundary)."""
from tests.kscan_cases import SCAN_KS, SCAN_STOPS

LONGEST_FIRST_KS = [0.20, 0.05, 0.10, 0.15, 0.15 + 0.05j, 0.18]
LONGEST_FIRST_STOPS = [400, 32, 43, 88, 104, 360]
assert sorted(LONGEST_FIRST_STOPS) == SCAN_STOPS and sorted(map(abs, LONGEST_FIRST_KS)) == sorted(map(abs, SCAN_KS))


def schedule(its, width, restart):
    """[(system, slot, step at which it is admitted)] and the number of lockstep steps"""
    free = [0] * min(width, len(its))          # the step at which the slot is (re)filled next
    out, end = [], 0
    for s, it in enumerate(its):
        j = min(range(len(free)), key=lambda q: (free[q], q))
        out.append((s, j, free[j]))
        free[j] = -(-(free[j] + it) // restart) * restart
        end = max(end, free[j])
    return out, end


def lockstep_steps(its, width, restart):
    return schedule(its, width, restart)[1]


def wait_for_group_steps(its, width, restart):
    """the policy the queue is NOT: the next `width` systems start when the whole group has stopped"""
    total = 0
    for g in range(0, len(its), width):
        total += -(-max(its[g:g + width]) // restart) * restart
    return total


# (its, width, lockstep steps with refill) at restart 5, max_iter 400 — computed by hand.  Waiting for the whole group instead would take
# 850 steps in the first case (400 + 90 + 360): it tells the two policies apart.
HAND = [
    (LONGEST_FIRST_STOPS, 2, 635),     # slot 1: 32 -> 35, 43 -> 80, 88 -> 170, 104 -> 275, 360 -> 635; slot 0 holds the 400
    (SCAN_STOPS, 3, 490),              # slot 0: 32 -> 35, 104 -> 140; slot 1: 43 -> 45, 360 -> 405; slot 2: 88 -> 90, 400 -> 490
    (SCAN_STOPS, 6, 400),
    (SCAN_STOPS, 1, 1035),             # 35 + 45 + 90 + 105 + 360 + 400
]
