"""The one-launch step kernels (csrc/gcr_stepbuild.hip) wait for each other inside a launch: every instantiation the 128^3 headline
launches must keep two 1024-thread workgroups per CU, i.e. 8 waves per SIMD (<= 64 VGPRs), and must not spill to scratch.
Checked on the code object hipcc builds for gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (up to 2 stored directions the default dispatch launches the kernels that read r once: sb_keep_fits)
HEADLINE = ["step_keep_kernel<1, true, false, true>", "step_keep_kernel<2, true, false, true>",
            "step_build_kernel<3, 7, 3, true, false, true>", "step_build_kernel<3, 7, 4, true, false, true>",
            "step_build_kernel<3, 7, 5, true, true, true>", "start_build_kernel<true>", "start_build_kernel<false>"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("regs") / "x.o"
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "gcr_stepbuild.hip", "-o", str(out)],
                         capture_output=True, text=True, cwd=CS, check=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
            cur = re.sub(r"\(.*", "", name).replace("void mgcr::", "")
            res[cur] = {}
            continue
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    return res


@pytest.mark.parametrize("kernel", HEADLINE)
def test_headline_step_kernels_fit(usage, kernel):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u
