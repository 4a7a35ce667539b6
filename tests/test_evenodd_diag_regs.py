"""Register budget of the kernels of the even-odd operator with a site diagonal (csrc/evenodd_diag.hip) on the code object hipcc
builds for gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed.  diag_stage2_kernel<MODE, WT, NDT> mirrors
schur_step_apply_kernel with one 16-byte stream and one complex product more per row (NDT = 0: the plain stage 2);
diag_stage1_kernel<MODE, WT> is the row product scaled by 1 / a_o.  The built kernels are exactly the dispatched ones; nothing
spills; the forms that mirror the 8-wave forms (dictionary with values, 7-slot stencil view, up to 5 directions) keep 64 VGPRs and
8 waves per SIMD; every form keeps 4 waves; the element-wise kernels are light."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORMS = [(0, 0), (0, 7), (1, 0), (1, 7), (2, 0), (2, 7), (3, 7), (3, 9)]      # (MODE, WT) diag_dispatch_form names
EIGHT_WAVES = [(1, 0), (1, 7), (3, 7)]
FND = 10
ELEMENTWISE = ["diag_coeff_kernel", "diag_scale_kernel", "diag_combine_kernel", "diag_split_scaled_kernel", "diag_merge_scaled_kernel"]
NOT_BUILT = []      # (MODE, WT, NDT) forms that could not be had without scratch: none — DESIGN.md §10 would have to name each


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("regs") / "evenodd_diag.o"
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "evenodd_diag.hip", "-o", str(out)],
                         capture_output=True, text=True, cwd=CS, check=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
            cur = re.sub(r"\(.*", "", name).replace("void mgcr::", "").replace("mgcr::", "")
            res[cur] = {}
            continue
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    return res


def stage1(mode, wt):
    return "diag_stage1_kernel<%d, %d>" % (mode, wt)


def stage2(mode, wt, ndt):
    return "diag_stage2_kernel<%d, %d, %d>" % (mode, wt, ndt)


def test_every_dispatched_form_is_built_and_no_other(usage):
    want = [stage2(m, w, n) for m, w in FORMS for n in range(0, FND + 1) if (m, w, n) not in NOT_BUILT]
    want += [stage1(m, w) for m, w in FORMS] + ELEMENTWISE
    assert sorted(usage) == sorted(want)


def test_forms_not_built_are_named_in_the_design_notes():
    txt = open(os.path.join(CS, "..", "..", "DESIGN.md")).read()
    sec = txt[txt.index("Site diagonal"):]
    for m, w, n in NOT_BUILT:
        assert stage2(m, w, n) in sec
    if not NOT_BUILT:
        assert "every form is built" in sec


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


@pytest.mark.parametrize("ndt", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode,wt", EIGHT_WAVES)
def test_up_to_five_directions_run_at_eight_waves(usage, mode, wt, ndt):
    if (mode, wt, ndt) in NOT_BUILT:
        assert stage2(mode, wt, ndt) not in usage
        return
    u = usage[stage2(mode, wt, ndt)]
    assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, u


@pytest.mark.parametrize("mode,wt", EIGHT_WAVES)
def test_stage1_of_the_eight_wave_forms_runs_at_eight_waves(usage, mode, wt):
    u = usage[stage1(mode, wt)]
    assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, u


@pytest.mark.parametrize("mode,wt", FORMS)
def test_every_form_keeps_four_waves_and_the_mirrored_lds(usage, mode, wt):
    u = usage[stage1(mode, wt)]
    assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128 and u["LDS Size [bytes/block]"] == 0, u
    for ndt in range(0, FND + 1):
        if (mode, wt, ndt) in NOT_BUILT:
            continue
        u = usage[stage2(mode, wt, ndt)]
        assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128, (ndt, u)      # one 1024-thread workgroup per CU at the least
        assert u["LDS Size [bytes/block]"] == 2 * ndt * 17 * 8, (ndt, u)             # block_sum_owner's scratch, nothing else static


def test_elementwise_kernels_are_light(usage):
    for k in ELEMENTWISE:
        assert usage[k]["VGPRs"] <= 32 and usage[k]["Occupancy [waves/SIMD]"] == 8, usage[k]
