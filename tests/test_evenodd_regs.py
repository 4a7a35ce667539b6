"""Register budget of the even-odd preconditioned DiracOp's kernels (csrc/evenodd.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  schur_step_apply_kernel<MODE, WT, NDT> — stage 2 of the Schur apply with a
GCR step's beta dot products — mirrors step_apply_kernel: in the forms that kernel runs at 8 waves per SIMD (dictionary with
values, 7-slot stencil view) it takes at most 64 VGPRs up to 5 directions, so that two 1024-thread workgroups share a CU; no form
spills to scratch at any direction count; the reduction scratch in LDS is that of the mirrored kernel."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORMS = [(0, 0), (0, 7), (1, 0), (1, 7), (2, 0), (2, 7), (3, 7), (3, 9)]      # (MODE, WT) the dispatch of eo_schur_step names
EIGHT_WAVES = [(1, 0), (1, 7), (3, 7)]
FND = 10


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("regs") / "evenodd.o"
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "evenodd.hip", "-o", str(out)],
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


def name(mode, wt, ndt):
    return "schur_step_apply_kernel<%d, %d, %d>" % (mode, wt, ndt)


def test_every_dispatched_form_is_built_and_no_other(usage):
    want = [name(m, w, n) for m, w in FORMS for n in range(1, FND + 1)] + ["eo_split_kernel", "eo_merge_kernel", "eo_sub_scaled_kernel"]
    assert sorted(usage) == sorted(want)


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


@pytest.mark.parametrize("ndt", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode,wt", EIGHT_WAVES)
def test_up_to_five_directions_run_at_eight_waves(usage, mode, wt, ndt):
    u = usage[name(mode, wt, ndt)]
    assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, u


@pytest.mark.parametrize("mode,wt", FORMS)
def test_every_form_keeps_four_waves_and_the_mirrored_lds(usage, mode, wt):
    for ndt in range(1, FND + 1):
        u = usage[name(mode, wt, ndt)]
        assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128, (ndt, u)      # one 1024-thread workgroup per CU at the least
        assert u["LDS Size [bytes/block]"] == 2 * ndt * 17 * 8, (ndt, u)             # block_sum_owner's scratch, nothing else static


def test_split_and_merge_are_light(usage):
    for k in ("eo_split_kernel", "eo_merge_kernel", "eo_sub_scaled_kernel"):
        assert usage[k]["VGPRs"] <= 32 and usage[k]["Occupancy [waves/SIMD]"] == 8, usage[k]
