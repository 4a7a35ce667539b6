"""The apply of step_keep_kernel and step_keep_wide_kernel (csrc/gcr_stepbuild_keep_body.h) takes, in the forms for real
coefficients, the row's own r from the stencil's diagonal gather (spmv_dev.h sten_row_product_own_t).  Every form the dispatch can
launch must still keep two 1024-thread workgroups per CU — 0 scratch, 8 waves per SIMD, <= 64 VGPRs — and the load the change
removes must be gone from the code: step_keep_kernel<1, true, false, true> had 54 global loads, 42 of them 16 bytes wide (4 trips x
(7 gathers + the own r) + 10 stream loads); it has 50 and 38 (4 trips x 7 gathers + the same 10).
With r[i - 1] and r[i + 1] from the neighbouring lanes as well (-DMGCR_SB_APPLY=2: 4 far gathers, the own r and one two-lane edge
load per trip) it has 46 and 34 = 4 x 6 + 10, and 32 one-dword whole-wave shifts; that form was measured slower than this one in
every kernel of the headline and is not built, so the count pinned here is the built form's.
Checked on the code hipcc builds for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_stepbuild_keep_all_regs import CS, HIPCC, KEEP, usage  # noqa: F401  (the module-scoped fixture: one compile for this file)
from tests.test_stepbuild_keep_wide_regs import WIDE


@pytest.mark.parametrize("kernel", KEEP + WIDE)
def test_dispatched_forms_fit(usage, kernel):  # noqa: F811
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u


@pytest.fixture(scope="module")
def keep1_asm(tmp_path_factory):
    """the gfx950 assembly of step_keep_kernel<1, true, false, true>"""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("asm") / "x.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "gcr_stepbuild.hip", "-o", str(out)], capture_output=True, text=True, cwd=CS, check=True)
    body, inside = [], False
    for line in out.read_text().splitlines():
        if line.startswith("_ZN4mgcr16step_keep_kernelILi1ELb1ELb0ELb1EEEvNS_13StepBuildArgsE:"):
            inside = True
        if inside:
            body.append(line)
            if "s_endpgm" in line:
                break
    assert body and "s_endpgm" in body[-1]
    return body


def test_the_apply_loads_seven_per_trip(keep1_asm):
    loads = [ln for ln in keep1_asm if re.search(r"^\s*global_load", ln)]
    wide = [ln for ln in loads if "global_load_dwordx4" in ln]
    assert (len(loads), len(wide)) == (50, 4 * 7 + 10), (len(loads), len(wide))
