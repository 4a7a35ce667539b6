"""The keep body of the one-launch GCR steps (csrc/gcr_stepbuild_keep_body.h) requests the operands of its scalar stage — the |r|^2
partials, den[], and at the close lc->cx and the coefficient table's columns — behind the apply and parks them in LDS, and keeps
per form as many rows of Ap_0 from the pass-1 dots to the build as fit (csrc/gcr_stepbuild.hip sb_kept_rows).  The workgroups of
such a launch wait for each other, so every step_keep_kernel / step_keep_wide_kernel form must still keep two 1024-thread
workgroups per CU — 0 scratch, 8 waves per SIMD, <= 64 VGPRs; the forms for complex coefficients, which the commit before built
with 0 scratch every one, must not need any either.  The kept-row table is pinned per form (static_assert on the constexpr
function), and a kept row is a 16-byte global load less in the code: counted on the commit before,
step_keep_kernel<2, true, false, true> had 48 such loads (2 rows kept), step_keep_kernel<3, true, false, true> 58 (2 rows) and
step_keep_wide_kernel<4, true, false, true> 70 (none); each keeps one row more and has 47, 57 and 69.  (The stage's own loads
do not change these counts: den[] was one 16-byte load per thread and still is.)
Checked on the code hipcc builds for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_stepbuild_keep_all_regs import CS, HIPCC, KEEP
from tests.test_stepbuild_keep_wide_regs import WIDE

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off"]


def _hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def _kept_rows(wide, nd, xr, close, realc):
    """the table: rows of Ap_0 a form keeps in registers across exchange 1"""
    if nd == 1:
        return 3
    if not realc:
        return 0 if wide else 2
    if not wide:
        return 4 if (close and not xr) else 3
    if nd == 4:
        return 4 if close else 1
    return 2 if xr else 3


def _parse(name):
    m = re.match(r"step_keep(_wide)?_kernel<(\d), (true|false), (true|false), (true|false)>", name)
    return (m.group(1) is not None, int(m.group(2))) + tuple(g == "true" for g in m.groups()[2:])


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """one device compile: {kernel: resource usage}, {kernel: its assembly lines}"""
    out = tmp_path_factory.mktemp("stage") / "x.s"
    err = subprocess.run([_hipcc()] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", "gcr_stepbuild.hip",
                                               "-o", str(out)], capture_output=True, text=True, cwd=CS, check=True).stderr

    def pretty(mangled):
        name = subprocess.check_output(["c++filt", mangled], text=True).strip()
        return re.sub(r"\(.*", "", name).replace("void mgcr::", "")

    usage, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = pretty(m.group(1))
            usage[cur] = {}
            continue
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                usage[cur][key] = int(m.group(1))
    asm, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"(_ZN4mgcr\d+step_keep\w+):", line)
        if m:
            cur = pretty(m.group(1))
            asm[cur] = []
        if cur is not None:
            asm[cur].append(line)
            if "s_endpgm" in line:
                cur = None
    return usage, asm


@pytest.mark.parametrize("kernel", KEEP + WIDE)
def test_every_form_fits_without_scratch(built, kernel):
    usage, _ = built
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 8, u
    assert u["VGPRs"] <= 64, u


def test_the_kept_row_table(tmp_path):
    """sb_kept_rows<WIDE, NDT, XR, CLOSE, REALC>() of every built form, as static_asserts behind the translation unit"""
    lines = ['#include "gcr_stepbuild.hip"']
    for k in KEEP + WIDE:
        wide, nd, xr, close, realc = _parse(k)
        args = ", ".join(str(v).lower() if isinstance(v, bool) else str(v) for v in (wide, nd, xr, close, realc))
        lines.append('static_assert(mgcr::sb_kept_rows<%s>() == %d, "%s");' % (args, _kept_rows(wide, nd, xr, close, realc), k))
    src = tmp_path / "table.hip"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([_hipcc()] + FLAGS + ["--cuda-host-only", "-fsyntax-only", "-I", os.path.abspath(CS), str(src)],
                       capture_output=True, text=True, cwd=CS)
    assert p.returncode == 0, p.stderr[-3000:]


# 16-byte global loads on the commit before, rows kept there
WIDE_LOADS_BEFORE = {"step_keep_kernel<2, true, false, true>": (48, 2),
                     "step_keep_kernel<3, true, false, true>": (58, 2),
                     "step_keep_wide_kernel<4, true, false, true>": (70, 0)}


@pytest.mark.parametrize("kernel", sorted(WIDE_LOADS_BEFORE))
def test_a_kept_row_is_a_load_less(built, kernel):
    _, asm = built
    before, kept_before = WIDE_LOADS_BEFORE[kernel]
    body = asm[kernel]
    assert body and "s_endpgm" in body[-1]
    wide = [ln for ln in body if re.search(r"^\s*global_load_dwordx4", ln)]
    added = _kept_rows(*_parse(kernel)) - kept_before
    print(kernel, "16-byte global loads:", len(wide), "before:", before, "rows added:", added)
    assert added == 1
    assert len(wide) == before - added, (len(wide), before, added)
