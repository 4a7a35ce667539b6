"""The late-r pair forms of the one-launch GCR steps (csrc/gcr_steppair_late.hip step_pair_late_kernel): step_pair_kernel's body
(csrc/gcr_steppair_body.h) under the policy that does not hold r of the thread's eight rows from the apply to the build — the build
loads it again — and keeps 8 to 9 thread-rows of the stored directions more in the registers that frees.  Its workgroups wait for
each other, so every built form must fit one workgroup per CU the way the host assumes: 0 scratch, <= 128 VGPRs, 4 waves per SIMD.
The translation unit holds exactly the three late forms (3 and 4 directions, the close at 5); the kept-row table
(sb_pair_late_kept) and the gate of the default dispatch (sb_pair_late_form) are pinned by static_asserts; a kept row is a 16-byte
global load less in the code (against the unit built with -DMGCR_SB_PAIR_LATE_KEPT=0); and the table is the maximum: with one row
more (-DMGCR_SB_PAIR_LATE_MORE=1) every form spills.  Counts loads only.
Checked on the code hipcc builds for gfx950; no GPU needed."""
import os
import re
import subprocess

import pytest

from tests.test_stepbuild_keep_all_regs import CS
from tests.test_stepbuild_pair_regs import FLAGS, _hipcc

# (stored directions, closing): thread-rows kept — the eight of Ap_0, the eight of Ap_1, then rows of Ap_2
KEPT = {(3, False): 22, (4, False): 20, (5, True): 20}
# the forms the default dispatch hands out (option step_build_pair_late = 1)
ENABLED = {(3, False): True, (4, False): True, (5, True): True}


def _name(nd, close):
    return "step_pair_late_kernel<%d, %s>" % (nd, "true" if close else "false")


def _compile(out, extra):
    """one device compile of the translation unit: {kernel: resource usage}, {kernel: number of 16-byte global loads}"""
    err = subprocess.run([_hipcc()] + FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", "gcr_steppair_late.hip",
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
    loads, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"(_ZN4mgcr\d+step_pair\w+):", line)
        if m:
            cur = pretty(m.group(1))
            loads[cur] = 0
        if cur is not None:
            if re.search(r"^\s*global_load_dwordx4", line):
                loads[cur] += 1
            if "s_endpgm" in line:
                cur = None
    return usage, loads


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("late") / "x.s", [])


@pytest.fixture(scope="module")
def built_none_kept(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("late0") / "x.s", ["-DMGCR_SB_PAIR_LATE_KEPT=0"])


@pytest.fixture(scope="module")
def built_one_more(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("late1") / "x.s", ["-DMGCR_SB_PAIR_LATE_MORE=1"])


@pytest.mark.parametrize("nd,close", sorted(KEPT))
def test_every_late_form_fits_one_workgroup_per_cu(built, nd, close):
    usage, _ = built
    assert _name(nd, close) in usage, sorted(usage)
    u = usage[_name(nd, close)]
    print(_name(nd, close), u)
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 4, u
    assert u["VGPRs"] <= 128, u


def test_the_unit_holds_exactly_the_late_forms(built):
    """every built form is in the library whatever the gate says (option 2 launches it), and nothing else is"""
    assert sorted(built[0]) == sorted(_name(nd, close) for nd, close in KEPT), sorted(built[0])


def test_the_kept_row_table_and_the_gate(tmp_path):
    lines = ['#include "gcr_steppair_late.hip"']
    for (nd, close), k in sorted(KEPT.items()):
        c = "true" if close else "false"
        lines.append('static_assert(mgcr::sb_pair_late_built<%d, %s>(), "built");' % (nd, c))
        lines.append('static_assert(mgcr::sb_pair_late_kept<%d, %s>() == %d, "kept rows");' % (nd, c, k))
        lines.append('static_assert(mgcr::sb_pair_late_form<%d, %s>() == %s, "gate");' % (nd, c, "true" if ENABLED[(nd, close)] else "false"))
    for nd in (1, 2, 5):
        lines.append('static_assert(!mgcr::sb_pair_late_built<%d, false>() && !mgcr::sb_pair_late_form<%d, false>(), "no late form in a cycle at 1, 2 and 5");' % (nd, nd))
    for nd in range(1, 5):
        lines.append('static_assert(!mgcr::sb_pair_late_built<%d, true>() && !mgcr::sb_pair_late_form<%d, true>(), "the closes below 5 directions keep their kernel");' % (nd, nd))
    src = tmp_path / "table.hip"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([_hipcc()] + FLAGS + ["--cuda-host-only", "-fsyntax-only", "-I", os.path.abspath(CS), str(src)],
                       capture_output=True, text=True, cwd=CS)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.parametrize("nd,close", sorted(KEPT))
def test_a_kept_row_is_a_load_less(built, built_none_kept, nd, close):
    loads, none = built[1][_name(nd, close)], built_none_kept[1][_name(nd, close)]
    print(_name(nd, close), "16-byte global loads:", loads, "with no row kept:", none, "rows kept:", KEPT[(nd, close)])
    assert none - loads == KEPT[(nd, close)], (none, loads)


@pytest.mark.parametrize("nd,close", sorted(KEPT))
def test_one_row_more_spills(built_one_more, nd, close):
    u = built_one_more[0][_name(nd, close)]
    print(_name(nd, close), "with one row more:", u)
    assert u["ScratchSize [bytes/lane]"] > 0, u
