"""The host decisions of the Sparse format build (csrc/spmv_layout.h: ELL width and lanes, tail dealing, window tail
tables, the two stages of the stencil-view analysis) on the CPU: tests/cpp/spmv_layout_check.cpp is built with g++ and
the address / undefined-behaviour sanitizers, run as a child process, and each line it prints is compared with the value
worked out by hand from the rules (the cost formula of choose_width, TAIL_CAP = 2048 entries and TAIL_THREADS = 256 rows
per chunk, 1024-row window tiles, STEN_MAX = 9, STEN_COMMON = 7, near slots within 256 / 512 rows, halo >= 32)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P7 = "off=-4096,-64,-1,0,1,64,4096 re=-1,-1,-1,6,-1,-1,-1 im=0,0,0,0,0,0,0"
NEAR64 = "near=0x3e halo=64 near_f=0x3e halo_f=64"   # the +-1 and +-64 slots (and the diagonal between them): kernel slots 1..5
LEAD = ("view=1 slot_of=0,1,2,3,4,5,6,8,7 kernel_ns=9 stride=16 rare=0x180 pre=1 " + NEAR64 + " reach=4096 "
        "off=-4096,-64,-1,0,1,64,4096,262144,8192 re=-1,-1,-1,6,-1,-1,-1,-1,-1 im=0,0,0,0,0,0,0,0,0 pmask=0x1ff,0xff,0x17f")
EXPECTED = [
    # cost(W) = 20 W nrow + 40 tail(W) + 64 tail_rows(W): 119 964 at 5, 10 010 000 at 500, 284 064 at 0
    "width skew W=5",
    "width flat W=7",
    "lanes 4 1 1",
    "tail mixed chunks={0,1,0,100}{2,4,3100,3300} long=1",
    "tail ones chunks={0,256,0,256}{256,300,256,300} long=",
    "tail cap chunks={0,1,0,2048} long=",
    "tail cap+1 chunks= long=0",
    "window tile_tail=0,1,2,3 row_tail=[5]=0[2499]=2 rows=2500",
    "stage1 laplace1d view=1 lead=0 S=-1,0,1 bits=0x7,0x6,0x3 re=-1,2,-1 im=0,0,0",
    "stage1 value-differs view=0",
    "stage1 descending view=0",
    "stage1 17-offsets view=0",
    "stage1 lead-and-ascending view=0",
    "stage1 lead view=1 lead=1 S=-1,0,5 bits=0x7,0x3 re=1,2,3 im=0,0,0",
    "stage2 poisson64 view=1 slot_of=0,1,2,3,4,5,6 kernel_ns=7 stride=8 rare=0x0 pre=0 " + NEAR64 + " reach=-1 " + P7 + " pmask=0x7f,0x7e",
    # +-1024 lies outside both windows; +-1 alone (halo < 32) is left to L1
    "stage2 poisson1024 view=1 slot_of=0,1,2,3,4,5,6 kernel_ns=7 stride=8 rare=0x0 pre=0 near=0x0 halo=0 near_f=0x0 halo_f=0 reach=-1 "
    "off=-1048576,-1024,-1,0,1,1024,1048576 re=-1,-1,-1,6,-1,-1,-1 im=0,0,0,0,0,0,0 pmask=0x7f",
    "stage2 force-rare view=1 slot_of=0,1,2,3,4,5,6 kernel_ns=9 stride=16 rare=0x180 pre=0 " + NEAR64 + " reach=4096 "
    "off=-4096,-64,-1,0,1,64,4096,0,0 re=-1,-1,-1,6,-1,-1,-1,0,0 im=0,0,0,0,0,0,0,0,0 pmask=0x7f,0x7e",
    # 4096 * 16 < 262144: both halo slots are rare -> kernel slots 7, 8; reach is that of the common slots
    "stage2 row-block view=1 slot_of=0,1,2,3,4,5,6,7,8 kernel_ns=9 stride=16 rare=0x180 pre=0 " + NEAR64 + " reach=4096 "
    "off=-4096,-64,-1,0,1,64,4096,8192,262144 re=-1,-1,-1,6,-1,-1,-1,-1,-1 im=0,0,0,0,0,0,0,0,0 pmask=0x7f,0xfe,0x17f",
    # leading slot (the largest offset) -> kernel slot 7, summed first; the rare slot behind the common ones -> 8
    "stage2 lead " + LEAD,
    # no slot rare by count, but eight in ascending position: the last of them is the ninth slot
    "stage2 ninth-slot " + LEAD,
    "stage2 lead-nine-ascending view=0",
]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spmv_layout") / "spmv_layout_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "spmv_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    return p.stdout.splitlines()


def test_every_case_printed_once(printed):
    assert [" ".join(l.split()[:2]) for l in printed] == [" ".join(l.split()[:2]) for l in EXPECTED]


@pytest.mark.parametrize("line", EXPECTED, ids=lambda l: "-".join(l.split()[:2]))
def test_layout_decision(printed, line):
    key = line.split()[:2]
    got = [l for l in printed if l.split()[:2] == key]
    assert got == [line]
