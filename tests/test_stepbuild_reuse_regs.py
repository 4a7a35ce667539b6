"""step_build_kernel's closing forms at 4 and 5 stored directions run the close pass and the build as one loop over the rows
(csrc/gcr_stepbuild.hip sb_close_merged).  The workgroups of a one-launch step wait for each other, so every instantiation the
dispatch can launch for real coefficients must still keep two 1024-thread workgroups per CU — 8 waves per SIMD, <= 64 VGPRs — and
no scratch; the complex-coefficient instantiations must not need more scratch than they did before the merged loop (0 everywhere
except <3, 7, 5, true, true, false>: 12 B per lane).  Checked on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage), with the compile and the parse of tests/test_stepbuild_keep_all_regs.py; no GPU needed."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _b(v):
    return "true" if v else "false"


FORMS = list(itertools.product(range(1, 6), (True, False), (True, False)))
REAL = ["step_build_kernel<3, 7, %d, %s, %s, true>" % (nd, _b(xr), _b(cl)) for nd, xr, cl in FORMS]
CPLX = ["step_build_kernel<3, 7, %d, %s, %s, false>" % (nd, _b(xr), _b(cl)) for nd, xr, cl in FORMS]
SCRATCH_BEFORE = {"step_build_kernel<3, 7, 5, true, true, false>": 12}   # bytes per lane; every other form: 0


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


def test_every_form_is_built(usage):
    built = sorted(k for k in usage if k.startswith("step_build_kernel<"))
    assert built == sorted(REAL + CPLX), built


@pytest.mark.parametrize("kernel", REAL)
def test_real_coefficient_forms_fit(usage, kernel):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u


@pytest.mark.parametrize("kernel", CPLX)
def test_complex_coefficient_forms_need_no_more_scratch(usage, kernel):
    assert kernel in usage, sorted(usage)
    assert usage[kernel]["ScratchSize [bytes/lane]"] <= SCRATCH_BEFORE.get(kernel, 0), usage[kernel]
