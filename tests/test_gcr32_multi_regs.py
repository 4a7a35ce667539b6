"""Register budget of the batched low-precision GCR's kernels (csrc/gcr32_multi.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed, resource usage only.  The built kernels are exactly the dispatched ones — the
apply for K = 1, 2, 4, 8, 16 columns on a real and on a complex slab; the dots for 1 .. 15 stored directions; the build for 0 .. 15;
the update; entry and exit with 1, 2 or 4 columns per thread; the x correction of the defect-correction loop —; nothing spills; every
form keeps 4 waves per SIMD (one 1024-thread workgroup per CU at the least); and the occupancy of every form is the one DESIGN.md
§11.2 records."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CS = os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_ND = 15         # restart <= 16: at most 15 directions are stored when a step starts
KS = (1, 2, 4, 8, 16)
KCS = (1, 2, 4)
# a form that cannot be had at 4 waves without scratch is capped — DESIGN.md §11.2 names it: more than 8 directions in one pass of the
# dots (30 double accumulators); the second 8 go to the workgroups of gridDim.z = 1 inside the same form
NOT_DISPATCHED = []

# waves per SIMD, as recorded in DESIGN.md §11.2 (rows of its register table)
OCC = {
    "apply<K, complex>": [8, 8, 8, 6, 5],
    "apply<K, real>": [8, 8, 8, 7, 5],
    "dots<ND>": [8, 8, 8, 8, 8, 7, 5, 5, 5, 5, 5, 5, 5, 5, 5],
    "build<ND>": [8, 8, 8, 8, 8, 8, 8, 8, 8, 7, 7, 7, 8, 8, 8, 8],
    "update": [8],
    "entry<KC>": [8, 8, 8],
    "exit<KC>": [8, 8, 8],
}


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
    return resource_usage("gcr32_multi.hip", tmp_path_factory.mktemp("regs") / "gcr32_multi.o")


def rows():
    """table row -> the kernels of that row, in the row's order"""
    out = {"apply<K, complex>": ["g32m_apply_kernel<%d, false>" % k for k in KS], "apply<K, real>": ["g32m_apply_kernel<%d, true>" % k for k in KS],
           "dots<ND>": ["g32m_dots_kernel<%d>" % nd for nd in range(1, MAX_ND + 1)],
           "build<ND>": ["g32m_build_kernel<%d>" % nd for nd in range(MAX_ND + 1)], "update": ["g32m_update_kernel"]}
    for name in ("entry", "exit"):
        out["%s<KC>" % name] = ["g32m_%s_kernel<%d>" % (name, kc) for kc in KCS]
    return out


def forms():
    return [f for fs in rows().values() for f in fs]


def test_every_dispatched_kernel_is_built_and_no_other(usage):
    assert sorted(usage) == sorted(forms() + ["g32m_correct_kernel"])
    assert not set(NOT_DISPATCHED) & set(usage)


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


def test_every_form_keeps_four_waves(usage):
    for f in forms() + ["g32m_correct_kernel"]:
        u = usage[f]
        assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128, (f, u)
        assert u["LDS Size [bytes/block]"] <= 40 * 17 * 8, (f, u)          # the fold's and the block sums' mirrors and the betas, nothing else


def test_occupancy_is_the_recorded_one(usage):
    got = {row: [usage[f]["Occupancy [waves/SIMD]"] for f in fs] for row, fs in rows().items()}
    assert got == OCC


def test_the_design_notes_record_the_table_and_name_the_capped_forms():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = txt[txt.index("### 11.2"):]
    for row, occ in OCC.items():
        assert "| `%s` | %s |" % (row, " ".join(str(o) for o in occ)) in sec, row
    assert "more than 8 directions" in sec and "gridDim.z" in sec
