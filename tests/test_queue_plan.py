"""The schedule of the queued batched GCR (csrc/queue_plan.h) on the CPU: tests/cpp/queue_plan_check.cpp is built with g++ and the
address / undefined-behaviour sanitizers and drives the schedule with a stand-in for the device (system s stops after its[s] steps);
what it prints is compared with the Python model of tests/queue_cases.py and with numbers computed by hand."""
import os
import subprocess

import pytest

from tests import queue_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("queue_plan") / "queue_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "queue_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return path


def run(exe, width, restart, max_iter, check_every, its):
    p = subprocess.run([exe] + [str(v) for v in [width, restart, max_iter, check_every] + list(its)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    lines = p.stdout.splitlines()
    last = lines[-1].split()
    summary = {last[i]: int(last[i + 1]) for i in range(0, len(last), 2)}
    admits = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("admit ")]
    retires = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("retire ")]
    resets = [int(l.split()[1]) for l in lines if l.startswith("reset ")]
    return summary, admits, retires, resets


def test_the_header_includes_no_hip():
    txt = open(os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc", "queue_plan.h")).read()
    assert "#include <hip" not in txt and '#include "internal.h"' not in txt


@pytest.mark.parametrize("its,width,steps", qc.HAND, ids=["longest-first-w2", "scan-w3", "scan-w6", "scan-w1"])
def test_hand_computed_cases(exe, its, width, steps):
    assert qc.lockstep_steps(its, width, 5) == steps                      # the model gives the number computed by hand ...
    summary, admits, retires, resets = run(exe, width, 5, 400, 5, its)
    assert summary["steps"] == steps                                      # ... and so does the C++ schedule
    assert admits == qc.schedule(its, width, 5)[0]
    assert summary["admissions"] == len(its) - min(width, len(its)) and not resets
    assert sorted(s for s, _, _ in retires) == list(range(len(its)))      # every system retired once
    if width == 2:                                                        # a schedule that waited for the whole group would take 850 steps
        assert qc.wait_for_group_steps(its, 2, 5) == 850 > summary["steps"]


MODEL = [
    ("tie", [10, 8, 20, 20, 5], 2, 5, 400, 5),                 # two slots stop at one boundary: systems 2, 3 into slots 0, 1 at step 10
    ("tie-w3", [15, 11, 14, 7, 7, 7, 30], 3, 5, 400, 5),
    ("width>nsys", [12, 33], 8, 5, 400, 5),
    ("nsys=1", [37], 4, 5, 400, 5),
    ("w16", list(range(1, 40)), 16, 4, 400, 4),
    ("check_every-2-restarts", [400, 32, 43, 88, 104, 360], 2, 5, 400, 10),   # the boundary polls refill; the check_every ones change nothing
    ("max_iter", [20, 20, 20, 20, 20], 2, 5, 20, 5),            # known stopped at the deadline, which is a boundary
]


@pytest.mark.parametrize("name,its,width,restart,max_iter,check_every", MODEL, ids=[m[0] for m in MODEL])
def test_schedule_equals_the_model(exe, name, its, width, restart, max_iter, check_every):
    summary, admits, retires, resets = run(exe, width, restart, max_iter, check_every, its)
    want, steps = qc.schedule(its, width, restart)
    assert admits == want and summary["steps"] == steps and not resets
    assert summary["admissions"] == len(its) - min(width, len(its))


def test_ties_fill_ascending_slots(exe):
    _, admits, _, _ = run(exe, 2, 5, 400, 5, [10, 8, 20, 20, 5])
    assert admits[2:4] == [(2, 0, 10), (3, 1, 10)]


def test_all_stopped_in_mid_cycle_resets_the_phase(exe):
    # max_iter 7, restart 5, one slot: every system ends at its deadline in mid-cycle (phase 2); the next is admitted AT ONCE
    summary, admits, _, resets = run(exe, 1, 5, 7, 5, [7, 7, 7])
    assert admits == [(0, 0, 0), (1, 0, 7), (2, 0, 14)] and resets == [7, 14] and summary["steps"] == 21
    assert summary["last_steps"] == 3 and summary["short_steps"] == 3
    # max_iter < restart (the cycle never closes): a group ends together at the deadline — an early stop is not seen before
    summary, admits, _, resets = run(exe, 2, 5, 3, 10, [1, 3, 2, 3, 3])
    assert admits == [(0, 0, 0), (1, 1, 0), (2, 0, 3), (3, 1, 3), (4, 0, 6)] and resets == [3, 6] and summary["steps"] == 9
    assert summary["short_steps"] == 3
    # converged columns found by a check_every poll in mid-cycle while systems wait; the reset cycles then close at 7, 12: both end at 11
    summary, admits, _, resets = run(exe, 2, 5, 400, 2, [1, 2, 9, 9])
    assert admits == [(0, 0, 0), (1, 1, 0), (2, 0, 2), (3, 1, 2)] and resets == [2] and summary["steps"] == 12


def test_a_last_step_beside_running_neighbours_is_a_full_step(exe):
    # slot 0 reaches max_iter = 20 at step 20 while slot 1 (admitted at 5) goes on: a last step, not a short one
    summary, _, _, _ = run(exe, 2, 5, 20, 5, [20, 3, 20])
    assert summary["last_steps"] == 2 and summary["short_steps"] == 1 and summary["steps"] == 25
