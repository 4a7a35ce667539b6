"""Register budget of the queued batched GCR's kernels (csrc/gcr_multi.hip: the q_* entries) on the code object hipcc builds for
gfx950 (-Rpass-analysis=kernel-resource-usage); no GPU needed.  None spills to scratch.  The step kernels that share a body with a
batched-solve entry (q_build_kernel / m_build_kernel, q_close_x_kernel / m_close_x_kernel) keep that entry's occupancy and LDS;
the KC-templated streaming kernels of retirement and admission reach the waves per SIMD of m_xr_kernel<KC> — except
q_admit_kernel<4>, which carries the 24 running sums of m_init_partials_kernel<4> and has its occupancy (DESIGN.md section 9,
"Queued solve": it runs once per admission point, not per step)."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SCALAR = ["q_finish_kernel", "q_coef_kernel", "q_scatter_kernel", "q_r0_kernel", "q_admit_state_kernel"]
SHARED_BODY = {"q_build_kernel": "m_build_kernel", "q_close_x_kernel": "m_close_x_kernel"}
STREAMING = ["q_retire_kernel", "q_admit_kernel"]
EXCEPTIONS = {"q_admit_kernel<4>": "m_init_partials_kernel<4>"}   # kernel -> the entry whose occupancy it has instead of m_xr_kernel's


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = tmp_path_factory.mktemp("regs") / "gcr_multi.o"
    err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "gcr_multi.hip", "-o", str(out)],
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


def test_every_queue_kernel_is_there_and_none_spills(usage):
    names = [n for n in usage if n.startswith("q_")]
    want = SCALAR + [k + "<%d>" % kc for k in list(SHARED_BODY) + STREAMING for kc in (1, 2, 4)]
    assert sorted(names) == sorted(want)
    for n in names:
        assert usage[n]["ScratchSize [bytes/lane]"] == 0, (n, usage[n])


@pytest.mark.parametrize("kc", [1, 2, 4])
def test_step_kernels_keep_the_batched_entries_budget(usage, kc):
    for q, m in SHARED_BODY.items():
        a, b = usage["%s<%d>" % (q, kc)], usage["%s<%d>" % (m, kc)]
        assert a["Occupancy [waves/SIMD]"] >= b["Occupancy [waves/SIMD]"], (q, kc, a, b)
        assert a["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"], (q, kc, a, b)


@pytest.mark.parametrize("kc", [1, 2, 4])
@pytest.mark.parametrize("kernel", STREAMING)
def test_streaming_kernels_reach_the_residual_updates_occupancy(usage, kernel, kc):
    name = "%s<%d>" % (kernel, kc)
    ref = EXCEPTIONS.get(name, "m_xr_kernel<%d>" % kc)
    assert usage[name]["Occupancy [waves/SIMD]"] >= usage[ref]["Occupancy [waves/SIMD]"], (name, usage[name], ref, usage[ref])
