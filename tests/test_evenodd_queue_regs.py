"""Register budget of the queued even-odd scan's kernels (csrc/evenodd_queue.hip, and the work-block sink of m_pending_x_kernel in
csrc/gcr_multi.hip) on the
code object hipcc builds for gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed.  The masked gather / scatter / copy
<KP lanes per row> and the block form of the retiring x update <KC columns per thread> are streaming kernels: none touches scratch
or LDS, and each keeps 8 waves per SIMD, so that two 1024-thread workgroups share a CU.

The feature reaches everything else through entries that existed before it.  Those compile to what they were: spmm.hip against
tests/golden/spmm_kernel_usage.json, and the q_ / m_ kernels of gcr_multi.hip and the eom_ kernels of evenodd_multi.hip against
tests/golden/queue_kernel_usage.json, recorded from the commit before the queued even-odd scan.  (The rows stand under the names of
the instantiations that have since replaced the queued solve's copies — m_build_kernel<KC, true> for q_build_kernel<KC>, and so on,
profiles/multi_fold_resource_usage.md — with the figures recorded then; the one figure that moved with the fold is the VGPR count of
the flush form of the pending-x kernel at KC = 2, 4: 24 and 42, which were 26 and 44.)"""
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
NEW = ["%s<%d>" % (k, kp) for k in ("eoq_gather_kernel", "eoq_scatter_kernel", "eoq_copy_kernel") for kp in (1, 2, 4, 8, 16)]
NEW_IN_GCR_MULTI = ["m_pending_x_kernel<%d, XBlock>" % kc for kc in (1, 2, 4)]


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
    d = tmp_path_factory.mktemp("regs")
    return {src: resource_usage(hipcc, src, d / (src + ".o")) for src in ("evenodd_queue.hip", "gcr_multi.hip", "evenodd_multi.hip")}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "queue_kernel_usage.json")) as f:
        return json.load(f)


def test_the_kernels_built_are_the_ones_dispatched(usage):
    assert sorted(usage["evenodd_queue.hip"]) == sorted(NEW)
    assert all(k in usage["gcr_multi.hip"] for k in NEW_IN_GCR_MULTI)


@pytest.mark.parametrize("kernel", NEW + NEW_IN_GCR_MULTI)
def test_new_kernels_stream(usage, kernel):
    u = usage["gcr_multi.hip" if kernel in NEW_IN_GCR_MULTI else "evenodd_queue.hip"][kernel]
    print(kernel, u)
    assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8 and u["VGPRs"] <= 64, u


def test_the_queue_and_the_batched_solve_compile_to_the_kernels_they_had(usage, recorded):
    now = usage["gcr_multi.hip"]
    want = {k: v for k, v in recorded.items() if k.startswith(("q_", "m_"))}
    assert len(want) >= 30
    assert sorted(k for k in now if k not in NEW_IN_GCR_MULTI) == sorted(want)
    for name in want:
        assert now[name] == want[name], (name, now[name], want[name])


def test_the_even_odd_block_kernels_compile_to_what_they_were(usage, recorded):
    now = usage["evenodd_multi.hip"]
    want = {k: v for k, v in recorded.items() if k.startswith("eom_")}
    assert sorted(now) == sorted(want) and len(want) == 13
    for name in want:
        assert now[name] == want[name], (name, now[name], want[name])


def test_the_k_wide_apply_compiles_to_the_kernels_it_had(hipcc, tmp_path_factory):
    with open(os.path.join(HERE, "golden", "spmm_kernel_usage.json")) as f:
        rec = json.load(f)
    now = resource_usage(hipcc, "spmm.hip", tmp_path_factory.mktemp("regs") / "spmm.o")
    assert sorted(now) == sorted(rec)
    for name in rec:
        assert now[name] == rec[name], (name, now[name], rec[name])
