"""step_keep_wide_kernel (csrc/gcr_stepbuild.hip) runs step_keep_kernel's body — r read once — at 4 stored directions with the
next residual update (inside a cycle: the step a restart-5 cycle spends 22 % of its time in; closing one: restart 4) and at the
close at 5 (with the update: 36 % of a restart-5 cycle; without: a nested solve's last close), real and complex coefficients.  Their workgroups wait for each other inside a launch like every one-launch
step's, so each instantiation the dispatch can launch (sb_keep_wide_fits) must keep two 1024-thread workgroups per CU — 8 waves per
SIMD, <= 64 VGPRs — and must not spill to scratch, and nothing else may be built under that name.  Checked on the code object hipcc
builds for gfx950, with the compile and the parse of tests/test_stepbuild_keep_all_regs.py; no GPU needed."""
import itertools

import pytest

from tests.test_stepbuild_keep_all_regs import _b, usage  # noqa: F401  (the module-scoped fixture: one compile for this file)


def _fits(nd, xr, close):
    return (nd == 4 and xr) or (nd == 5 and close)


WIDE = [f"step_keep_wide_kernel<{nd}, {_b(xr)}, {_b(cl)}, {_b(rc)}>"
        for nd, xr, cl, rc in itertools.product(range(1, 6), (True, False), (True, False), (True, False)) if _fits(nd, xr, cl)]


def test_the_dispatch_names_eight_forms():
    assert len(WIDE) == 8, WIDE


def test_every_dispatched_form_is_built_and_no_other(usage):  # noqa: F811
    built = sorted(k for k in usage if k.startswith("step_keep_wide_kernel<"))
    assert built == sorted(WIDE), built


@pytest.mark.parametrize("kernel", WIDE)
def test_keep_wide_step_kernels_fit(usage, kernel):  # noqa: F811
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u
