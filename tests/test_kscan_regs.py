"""Register budget of the per-column-shift entries of the k-wide apply (csrc/spmm.hip, the *_kcol kernels a MultiDiracOp launches)
on the code object hipcc builds for gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed.  Each has a uniform-shift
counterpart of the same template arguments (tests/test_multi_rhs_regs.py lists those): it uses no scratch either and reaches
the counterpart's occupancy — the 16 shifts are read from the kernel arguments as scalars and cost no vector register."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FAMILIES = {"ell_multi_kernel": 20, "tail_chunk_multi_kernel": 3, "tail_long_multi_kernel": 4, "rowgen_multi_kernel": 5}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("regs") / "spmm.o"
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "spmm.hip", "-o", str(out)],
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


def pairs(usage):
    for name in usage:
        m = re.match(r"(\w+)_kcol(<.*>)$", name)
        if m:
            yield name, m.group(1) + m.group(2)


def test_every_per_column_entry_has_its_uniform_counterpart(usage):
    got = {}
    for kcol, uni in pairs(usage):
        assert uni in usage, (kcol, uni)
        fam = uni.split("<")[0]
        got[fam] = got.get(fam, 0) + 1
    assert got == FAMILIES, got


def test_per_column_entries_do_not_spill_and_keep_the_occupancy(usage):
    for kcol, uni in pairs(usage):
        a, b = usage[kcol], usage[uni]
        assert a["ScratchSize [bytes/lane]"] == 0, (kcol, a)
        assert a["Occupancy [waves/SIMD]"] >= b["Occupancy [waves/SIMD]"], (kcol, a, b)
        assert a["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"], (kcol, a, b)
