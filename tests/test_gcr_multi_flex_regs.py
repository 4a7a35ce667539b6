"""Register budget of the flexible batched GCR's kernels (csrc/gcr_multi_flex.hip) on the code object hipcc builds for gfx950
(-Rpass-analysis=kernel-resource-usage); no GPU needed, resource usage only.  The built kernels are exactly the dispatched ones — the
gate; the masked exit and the masked copy with 1, 2 or 4 columns per thread (mv_group's values) —; nothing spills; every form keeps
at least 4 waves per SIMD; and the occupancy of every form is the one DESIGN.md §11.3 records."""
import os

import pytest

from tests.test_gcr32_multi_regs import HIPCC, resource_usage

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KCS = (1, 2, 4)

# waves per SIMD, as recorded in DESIGN.md §11.3 (rows of its register table)
OCC = {
    "mflex_gate": [8],
    "mflex_exit<KC>": [8, 8, 8],
    "mflex_take<KC>": [8, 8, 8],
}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import shutil
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    return resource_usage("gcr_multi_flex.hip", tmp_path_factory.mktemp("regs") / "gcr_multi_flex.o")


def rows():
    return {"mflex_gate": ["mflex_gate_kernel"],
            "mflex_exit<KC>": ["mflex_exit_kernel<%d>" % kc for kc in KCS],
            "mflex_take<KC>": ["mflex_take_kernel<%d>" % kc for kc in KCS]}


def forms():
    return [f for fs in rows().values() for f in fs]


def test_every_dispatched_kernel_is_built_and_no_other(usage):
    assert sorted(usage) == sorted(forms())


def test_no_kernel_spills(usage):
    for n, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)


def test_every_form_keeps_four_waves(usage):
    for f in forms():
        u = usage[f]
        assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 128, (f, u)
        assert u["LDS Size [bytes/block]"] <= 8 * 17 * 8, (f, u)               # the fold's mirrors (2 scalars per column of a group), nothing else


def test_occupancy_is_the_recorded_one(usage):
    got = {row: [usage[f]["Occupancy [waves/SIMD]"] for f in fs] for row, fs in rows().items()}
    assert got == OCC


def test_the_design_notes_record_the_table():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = txt[txt.index("### 11.3"):]
    for row, occ in OCC.items():
        assert "| `%s` | %s |" % (row, " ".join(str(o) for o in occ)) in sec, row
