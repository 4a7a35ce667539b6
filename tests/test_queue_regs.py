"""Register budget of the queued batched GCR's kernels (csrc/gcr_multi.hip: the q_* entries, the QUEUED = true instantiations of the
kernels it shares with the batched solve, and the Field sink of the pending-x kernel) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed.  None spills to scratch.  The step kernels' queued instantiations
(m_build_kernel<KC, true>, m_close_x_kernel<KC, true>) keep the occupancy and LDS of the batched ones (<KC, false>); the
KC-templated streaming kernels of retirement and admission reach the waves per SIMD of m_xr_kernel<KC> — except
m_init_partials_kernel<4, true>, which carries the 24 running sums of m_init_partials_kernel<4, false> and has its occupancy
("Queued solve": it runs once per admission point, not per step)."""
import os
import re
import shutil
import subprocess

import pytest

CS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SCALAR = ["m_finish_kernel<true>", "m_coef_kernel<true>", "q_scatter_kernel", "q_r0_kernel", "q_admit_state_kernel"]
SHARED_BODY = {"m_build_kernel<%d, true>": "m_build_kernel<%d, false>", "m_close_x_kernel<%d, true>": "m_close_x_kernel<%d, false>"}
STREAMING = {"retire": "m_pending_x_kernel<%d, XFields>", "admit": "m_init_partials_kernel<%d, true>"}
# kernel -> the entry whose occupancy it has instead of m_xr_kernel's
EXCEPTIONS = {"m_init_partials_kernel<4, true>": "m_init_partials_kernel<4, false>"}


def is_queue_entry(name):
    return name.startswith("q_") or name.endswith("true>") or name.endswith("XFields>")


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
    names = [n for n in usage if is_queue_entry(n)]
    want = SCALAR + [k % kc for k in list(SHARED_BODY) + list(STREAMING.values()) for kc in (1, 2, 4)]
    assert sorted(names) == sorted(want)
    for n in names:
        assert usage[n]["ScratchSize [bytes/lane]"] == 0, (n, usage[n])


@pytest.mark.parametrize("kc", [1, 2, 4])
def test_step_kernels_keep_the_batched_entries_budget(usage, kc):
    for q, m in SHARED_BODY.items():
        a, b = usage[q % kc], usage[m % kc]
        assert a["Occupancy [waves/SIMD]"] >= b["Occupancy [waves/SIMD]"], (q, kc, a, b)
        assert a["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"], (q, kc, a, b)


@pytest.mark.parametrize("kc", [1, 2, 4])
@pytest.mark.parametrize("point", sorted(STREAMING))
def test_streaming_kernels_reach_the_residual_updates_occupancy(usage, point, kc):
    name = STREAMING[point] % kc
    ref = EXCEPTIONS.get(name, "m_xr_kernel<%d>" % kc)
    assert usage[name]["Occupancy [waves/SIMD]"] >= usage[ref]["Occupancy [waves/SIMD]"], (name, usage[name], ref, usage[ref])
