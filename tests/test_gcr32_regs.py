"""Register budget of the low-precision GCR's kernels (csrc/gcr32.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  The built kernels are exactly the dispatched ones — the apply for 0 .. 15
stored directions on a real and on a complex slab, the build for 0 .. 15, entry, update and exit —; nothing spills; every form keeps
4 waves per SIMD (one 1024-thread workgroup per CU at the least) and the forms for up to 5 stored directions, entry, update and exit
keep 8: the bar blk_combine_kernel is held to."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_ND = 15         # restart <= 16: at most 15 directions are stored when a step starts
NOT_BUILT = []      # forms that could not be had at 4 waves without scratch: none — DESIGN.md §11 would have to name each
STREAMING = ["g32_entry_kernel", "g32_update_kernel", "g32_exit_kernel"]


def resource_usage(src, out):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
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
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    return res


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return resource_usage("gcr32.hip", tmp_path_factory.mktemp("regs") / "gcr32.o")


def apply_k(nd, real):
    return "g32_apply_kernel<%d, %s>" % (nd, "true" if real else "false")


def build_k(nd):
    return "g32_build_kernel<%d>" % nd


def forms():
    return [apply_k(n, r) for n in range(MAX_ND + 1) for r in (False, True)] + [build_k(n) for n in range(MAX_ND + 1)]


def test_every_dispatched_kernel_is_built_and_no_other(usage):
    want = [f for f in forms() if f not in NOT_BUILT] + STREAMING
    assert sorted(usage) == sorted(want)


def test_forms_not_built_are_named_in_the_design_notes():
    txt = open(os.path.join(CS, "..", "..", "DESIGN.md")).read()
    sec = txt[txt.index("## 11."):]
    for f in NOT_BUILT:
        assert f in sec
    if not NOT_BUILT:
        assert "every form of g32_apply_kernel and g32_build_kernel is built" in sec


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


@pytest.mark.parametrize("nd", [0, 1, 2, 3, 4, 5])
def test_up_to_five_directions_run_at_eight_waves(usage, nd):
    for f in (apply_k(nd, False), apply_k(nd, True), build_k(nd)):
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


def test_streaming_kernels_are_light(usage):
    for k in STREAMING:
        assert usage[k]["VGPRs"] <= 64 and usage[k]["Occupancy [waves/SIMD]"] == 8, (k, usage[k])
