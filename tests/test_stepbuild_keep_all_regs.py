"""The one-launch steps that read r once (csrc/gcr_stepbuild.hip step_keep_kernel, option "step_build_keep_all") wait for each
other inside a launch like step_build_kernel: every instantiation the dispatch can launch (sb_keep_fits: up to 2 stored
directions in every form, 3 except the closing step with the next residual update; real and complex coefficients) must keep two
1024-thread workgroups per CU — 8 waves per SIMD, <= 64 VGPRs — and must not spill to scratch.  Checked on the code object hipcc
builds for gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _fits(nd, xr, close):
    return nd <= 2 or (nd == 3 and not (xr and close))


def _b(v):
    return "true" if v else "false"


KEEP = [f"step_keep_kernel<{nd}, {_b(xr)}, {_b(cl)}, {_b(rc)}>"
        for nd, xr, cl, rc in itertools.product(range(1, 6), (True, False), (True, False), (True, False)) if _fits(nd, xr, cl)]


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


def test_every_fitting_form_is_built(usage):
    built = sorted(k for k in usage if k.startswith("step_keep_kernel<"))
    assert built == sorted(KEEP), built


@pytest.mark.parametrize("kernel", KEEP)
def test_keep_all_step_kernels_fit(usage, kernel):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u
