"""The partition plan of a distributed operator (csrc/comm_plan.h: owners, symmetric peer lists, send lists in the peer's halo
order, local column numbering, the interior range, the block-to-element expansion, the send-list analysis, the layout of a
peer-write receive buffer, the sequence numbers) on the CPU: tests/cpp/comm_plan_check.cpp plays all ranks in one process, is
built with g++ and the address / undefined-behaviour sanitizers, run as a child process, and each line it prints is compared
with the value worked out by hand.  Per rank: offsets (first row of every rank, then n), halo (global ids), peers,
counts = (entries received, rows sent) @ start in the halo segment, send = local rows per peer, cols = local column numbers
(remote: nloc + halo slot), interior = longest run of rows without a halo column."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows 0-3, 4-7, 8-11 of the 12-point 3-point Laplacian: local columns of the first, a middle and the last block
C_FIRST, C_MID, C_LAST = "0,1,0,1,2,1,2,3,2,3,4", "4,0,1,0,1,2,1,2,3,2,3,5", "4,0,1,0,1,2,1,2,3,2,3"
EXPECTED = [
    "lap1d-3 rank0 offsets=0,4,8,12 halo=4 peers=1 counts=(1,1)@0 send={3} cols=" + C_FIRST + " interior=[0,3)",
    "lap1d-3 rank1 offsets=0,4,8,12 halo=3,8 peers=0,2 counts=(1,1)@0(1,1)@1 send={0}{3} cols=" + C_MID + " interior=[1,3)",
    "lap1d-3 rank2 offsets=0,4,8,12 halo=7 peers=1 counts=(1,1)@0 send={0} cols=" + C_LAST + " interior=[1,4)",
    # rank 1 owns no row: row 4 belongs to rank 2, the empty rank has no peers and an empty interior
    "lap1d-empty rank0 offsets=0,4,4,8,12 halo=4 peers=2 counts=(1,1)@0 send={3} cols=" + C_FIRST + " interior=[0,3)",
    "lap1d-empty rank1 offsets=0,4,4,8,12 halo= peers= counts= send= cols= interior=[0,0)",
    "lap1d-empty rank2 offsets=0,4,4,8,12 halo=3,8 peers=0,3 counts=(1,1)@0(1,1)@1 send={0}{3} cols=" + C_MID + " interior=[1,3)",
    "lap1d-empty rank3 offsets=0,4,4,8,12 halo=7 peers=2 counts=(1,1)@0 send={0} cols=" + C_LAST + " interior=[1,4)",
    # identity on 6 rows + entry (0, 5): rank 0 receives from rank 2 and sends it nothing; both list each other
    "one-sided rank0 offsets=0,2,4,6 halo=5 peers=2 counts=(1,0)@0 send={} cols=0,2,1 interior=[1,2)",
    "one-sided rank1 offsets=0,2,4,6 halo= peers= counts= send= cols=0,1 interior=[0,2)",
    "one-sided rank2 offsets=0,2,4,6 halo= peers=0 counts=(0,1)@0 send={1} cols=0,1 interior=[0,2)",
    # row 0 = columns 7, 0, 5, 7: halo unique and ascending, both 7s in slot 1
    "unsorted rank0 offsets=0,4,8 halo=5,7 peers=1 counts=(2,0)@0 send={} cols=5,0,4,5,1,2,3 interior=[1,4)",
    "unsorted rank1 offsets=0,4,8 halo= peers=0 counts=(0,2)@0 send={1,3} cols=0,1,2,3 interior=[0,4)",
    # runs [0, 2) and [3, 5): the first one wins
    "tie rank0 offsets=0,5,10 halo=5 peers=1 counts=(1,0)@0 send={} cols=0,1,2,5,3,4 interior=[0,2)",
    "tie rank1 offsets=0,5,10 halo= peers=0 counts=(0,1)@0 send={0} cols=0,1,2,3,4 interior=[0,5)",
    "all-touch rank0 offsets=0,2,4 halo=2,3 peers=1 counts=(2,0)@0 send={} cols=0,2,1,3 interior=[0,0)",
    "all-touch rank1 offsets=0,2,4 halo= peers=0 counts=(0,2)@0 send={0,1} cols=0,1 interior=[0,2)",
    "col-range error mgcr_plan_create: column 4 out of range",
    "unordered error mgcr_plan_create: row blocks must be ordered by rank and contiguous",
    "send-rows owned '' rows=1,3",
    "send-rows foreign 'mgcr_plan_create: peer asked for a row this rank does not own'",
    # lap1d-3 with 3 x 3 blocks: every number of the block plan times 3, lists expanded in order; same = equal to the element matrix's plan
    "expand rank0 same=1 offsets=0,12,24,36 halo=12,13,14 peers=1 counts=(3,3)@0 send={9,10,11} cols= interior=[0,9)",
    "expand rank1 same=1 offsets=0,12,24,36 halo=9,10,11,24,25,26 peers=0,2 counts=(3,3)@0(3,3)@3 send={0,1,2}{9,10,11} cols= interior=[3,9)",
    "expand rank2 same=1 offsets=0,12,24,36 halo=21,22,23 peers=1 counts=(3,3)@0 send={0,1,2} cols= interior=[3,12)",
    # rows 2,3,4 | 1,3 | 5 | none: contiguous from 2, a gap, a single row, an empty list
    "sendlists mixed off=0,3,5,6 cnt=3,2,1,0 contig=2,-1,5,-1 idx=2,3,4,1,3,5",
    "layout slot_bytes 0 256 256 512",    # 0, 1, 16, 17 entries of 16 bytes, rounded up to 256
    # 17 entries, 16 ranks: flags start at 2 * 512; slot 1's block 16 * 8 bytes further; 2 * 16 flag words in all
    "layout offsets slot=0,512 flag_rank3=1048,1176 total=1280",
    "seq advance 1 4294967295 2",
    "seq wrap 4294967294:0 4294967295:1 2:0 3:1 4:0",   # from 0xFFFFFFFD: the parity keeps alternating across the wrap
]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("comm_plan") / "comm_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "comm_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    return p.stdout.splitlines()


def test_every_case_printed_once(printed):
    assert [" ".join(l.split()[:2]) for l in printed] == [" ".join(l.split()[:2]) for l in EXPECTED]


@pytest.mark.parametrize("line", EXPECTED, ids=lambda l: "-".join(l.split()[:2]))
def test_plan_stage(printed, line):
    key = line.split()[:2]
    got = [l for l in printed if l.split()[:2] == key]
    assert got == [line]
