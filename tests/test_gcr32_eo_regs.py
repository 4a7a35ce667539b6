"""Register budget of the even-odd low-precision GCR's kernels (csrc/gcr32_eo.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  The bars are those of tests/test_gcr32_regs.py: the built kernels are exactly
the dispatched ones — stage 1 on a real and on a complex slab, with and without a diagonal, stage 2 for 0 .. 15 stored directions in the
same four forms —; nothing spills; stage 1 and stage 2 up to 5 stored directions keep 8 waves per SIMD, every form at least 4; LDS holds
only the fold's and the block sums' mirrors."""
import os

import pytest

from tests.test_gcr32_regs import CS, HIPCC, MAX_ND, resource_usage

NOT_BUILT = []      # forms that could not be had at 4 waves without scratch: none — DESIGN.md §11 would have to name each
FLAGS = [(r, d) for r in ("false", "true") for d in ("false", "true")]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import shutil
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return resource_usage("gcr32_eo.hip", tmp_path_factory.mktemp("regs") / "gcr32_eo.o")


def stage1_k(real, diag):
    return "g32_eo_stage1_kernel<%s, %s>" % (real, diag)


def stage2_k(nd, real, diag):
    return "g32_eo_stage2_kernel<%d, %s, %s>" % (nd, real, diag)


def forms():
    return [stage1_k(r, d) for r, d in FLAGS] + [stage2_k(n, r, d) for n in range(MAX_ND + 1) for r, d in FLAGS]


def test_every_dispatched_kernel_is_built_and_no_other(usage):
    assert sorted(usage) == sorted(f for f in forms() if f not in NOT_BUILT)


def test_forms_not_built_are_named_in_the_design_notes():
    txt = open(os.path.join(CS, "..", "..", "DESIGN.md")).read()
    sec = txt[txt.index("## 11."):]
    for f in NOT_BUILT:
        assert f in sec
    if not NOT_BUILT:
        assert "every form of g32_eo_stage1_kernel and g32_eo_stage2_kernel is built" in sec


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


def test_stage_1_runs_at_eight_waves(usage):
    for r, d in FLAGS:
        u = usage[stage1_k(r, d)]
        assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, (r, d, u)
        assert u["LDS Size [bytes/block]"] <= 2 * 17 * 8, (r, d, u)


@pytest.mark.parametrize("nd", [0, 1, 2, 3, 4, 5])
def test_stage_2_up_to_five_directions_runs_at_eight_waves(usage, nd):
    for r, d in FLAGS:
        f = stage2_k(nd, r, d)
        if f in NOT_BUILT:
            assert f not in usage
            continue
        u = usage[f]
        assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, (f, u)


def test_every_form_keeps_four_waves(usage):
    for f in forms():
        if f in NOT_BUILT:
            continue
        u = usage[f]
        assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128, (f, u)
        assert u["LDS Size [bytes/block]"] <= 32 * 17 * 8, (f, u)          # the fold's and the block sums' mirrors, nothing else
