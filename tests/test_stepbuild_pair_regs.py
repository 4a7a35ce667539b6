"""The pair forms of the one-launch GCR steps (csrc/gcr_steppair.hip step_pair_kernel): one 1024-thread workgroup per CU carries two
logical workgroups and keeps thread-rows of Ap_0 and Ap_1 in registers from the pass-1 dots to the build.  Its workgroups wait for
each other, so every built form must fit one workgroup per CU the way the host assumes: 0 scratch, <= 128 VGPRs, 4 waves per
SIMD — checked on all five, built with -DMGCR_SB_PAIR_FORMS=1 as for a measurement; the default build instantiates the
enabled ones only.  The kept-row table (sb_pair_kept) and the gate of the default dispatch (sb_pair_form) are pinned by static_asserts, and a
kept row is a 16-byte global load less in the code: the same translation unit built with no kept row (-DMGCR_SB_PAIR_KEPT=0) has
exactly as many such loads more as the form keeps rows; the form at 1 direction, whose eight rows of Ap_0 are all there is to keep,
has 8 x (7 gathers + 1 pass-1 row) + 1 operand of the scalar stage and none in its build.  Counts loads only.
Checked on the code hipcc builds for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_stepbuild_keep_all_regs import CS, HIPCC

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off"]
# (stored directions, closing): thread-rows kept — the eight of Ap_0, then rows of Ap_1
KEPT = {(1, False): 8, (2, False): 15, (3, False): 14, (4, False): 11, (5, True): 12}
# the forms the default dispatch hands out (all of them carry the next residual update)
ENABLED = {(1, False): False, (2, False): True, (3, False): True, (4, False): True, (5, True): False}


def _hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


def _name(nd, close):
    return "step_pair_kernel<%d, %s>" % (nd, "true" if close else "false")


def _compile(out, extra):
    """one device compile of the translation unit: {kernel: resource usage}, {kernel: number of 16-byte global loads}"""
    err = subprocess.run([_hipcc()] + FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", "gcr_steppair.hip",
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
    return _compile(tmp_path_factory.mktemp("pair") / "x.s", ["-DMGCR_SB_PAIR_FORMS=1"])


@pytest.fixture(scope="module")
def built_none_kept(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("pair0") / "x.s", ["-DMGCR_SB_PAIR_FORMS=1", "-DMGCR_SB_PAIR_KEPT=0"])


@pytest.mark.parametrize("nd,close", sorted(KEPT))
def test_every_form_fits_one_workgroup_per_cu(built, nd, close):
    usage, _ = built
    assert _name(nd, close) in usage, sorted(usage)
    u = usage[_name(nd, close)]
    assert u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 4, u
    assert u["VGPRs"] <= 128, u


def test_only_the_headline_forms_are_built(built):
    assert sorted(built[0]) == sorted(_name(nd, close) for nd, close in KEPT), sorted(built[0])


def test_the_default_build_holds_the_enabled_forms(tmp_path):
    usage, _ = _compile(tmp_path / "d.s", [])
    assert sorted(usage) == sorted(_name(nd, close) for (nd, close), on in ENABLED.items() if on), sorted(usage)


def test_the_kept_row_table_and_the_gate(tmp_path):
    lines = ['#include "gcr_steppair.hip"']
    for (nd, close), k in sorted(KEPT.items()):
        c = "true" if close else "false"
        lines.append('static_assert(mgcr::sb_pair_kept<%d, %s>() == %d, "kept rows");' % (nd, c, k))
        lines.append('static_assert(mgcr::sb_pair_form<%d, true, %s>() == %s, "gate");' % (nd, c, "true" if ENABLED[(nd, close)] else "false"))
        lines.append('static_assert(!mgcr::sb_pair_form<%d, false, %s>(), "no pair form without the next residual update");' % (nd, c))
    for nd in range(1, 5):
        lines.append('static_assert(!mgcr::sb_pair_form<%d, true, true>(), "the closes below 5 directions keep their kernel");' % nd)
    lines.append('static_assert(!mgcr::sb_pair_form<5, true, false>(), "5 directions inside a longer cycle keep their kernel");')
    src = tmp_path / "table.hip"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run([_hipcc()] + FLAGS + ["--cuda-host-only", "-fsyntax-only", "-I", os.path.abspath(CS), str(src)],
                       capture_output=True, text=True, cwd=CS)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.parametrize("nd,close", sorted(KEPT))
def test_a_kept_row_is_a_load_less(built, built_none_kept, nd, close):
    loads, none = built[1][_name(nd, close)], built_none_kept[1][_name(nd, close)]
    print(_name(nd, close), "16-byte global loads:", loads, "with no row kept:", none, "rows kept:", KEPT[(nd, close)])
    if nd == 1:   # (the macro leaves this form alone)
        assert loads == none == 8 * (7 + 1) + 1, (loads, none)
    else:
        assert none - loads == KEPT[(nd, close)], (none, loads)
