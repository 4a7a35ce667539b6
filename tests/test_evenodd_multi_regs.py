"""Register budget of the even-odd scan's kernels (csrc/evenodd_multi.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  The block split / merge <KP lanes per row> and the per-column
y = w - c u <KC columns per thread> are streaming kernels: none may touch scratch, and each keeps the 8 waves per SIMD recorded
here, so that two 1024-thread workgroups share a CU.

The operator reaches the k-wide apply of csrc/spmm.hip through entries that existed before it (every *_kcol kernel with w set):
spmm.hip compiles to the same kernels with the same registers, scratch, LDS and occupancy as recorded in
tests/golden/spmm_kernel_usage.json before the operator was added."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CS = os.path.join(HERE, "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
# kernel -> waves per SIMD
OCC = {"eom_split_kernel<%d>" % kp: 8 for kp in (1, 2, 4, 8, 16)}
OCC.update({"eom_merge_kernel<%d>" % kp: 8 for kp in (1, 2, 4, 8, 16)})
OCC.update({"eom_sub_scaled_kernel<%d>" % kc: 8 for kc in (1, 2, 4)})


def resource_usage(hipcc, src, out):
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(out)],
                         capture_output=True, text=True, cwd=CS, check=True).stderr
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.check_output(["c++filt", m.group(1)], text=True).strip()
            cur = re.sub(r"\(.*", "", name).replace("void mgcr::", "").replace("mgcr::", "")
            res[cur] = {}
            continue
        for key in KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def usage(hipcc, tmp_path_factory):
    return resource_usage(hipcc, "evenodd_multi.hip", tmp_path_factory.mktemp("regs") / "evenodd_multi.o")


def test_the_kernels_built_are_the_ones_dispatched(usage):
    assert sorted(usage) == sorted(OCC)


def test_no_new_kernel_uses_scratch(usage):
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (name, u)
        assert u["LDS Size [bytes/block]"] == 0, (name, u)


@pytest.mark.parametrize("kernel", sorted(OCC))
def test_occupancy_of_the_new_kernels(usage, kernel):
    print(kernel, usage[kernel])
    assert usage[kernel]["Occupancy [waves/SIMD]"] == OCC[kernel] and usage[kernel]["VGPRs"] <= 64, usage[kernel]


def test_the_k_wide_apply_compiles_to_the_kernels_it_had(hipcc, tmp_path_factory):
    with open(os.path.join(HERE, "golden", "spmm_kernel_usage.json")) as f:
        recorded = json.load(f)
    now = resource_usage(hipcc, "spmm.hip", tmp_path_factory.mktemp("regs") / "spmm.o")
    assert sorted(now) == sorted(recorded)
    for name in recorded:
        assert now[name] == recorded[name], (name, now[name], recorded[name])
