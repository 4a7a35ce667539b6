"""Which kernel form the fused GCR apply launchers (csrc/gcr_fused.hip) select for an operator (csrc/fused_form.h), on the
CPU: tests/cpp/fused_form_check.cpp is built with g++ and the address / undefined-behaviour sanitizers, run as a child
process, and each line it prints is compared with the form written out by hand from the launchers' table:

    operator                  step apply / init apply        xr step
    windowed regime, rare     tile<9, rare>                  error
    windowed regime, 7 slots  tile<7, not rare>              tile<7, not rare> if carried and A p is at hand, else error
    stencil, rare             plain<4, 9>                    the same
    stencil, 7 slots          plain<3, 7>                    the same
    stencil, other            plain<3, 9>                    the same
    pat_mode 1 / 2 / 0        plain<mode, W == 7 ? 7 : 0>    the same      (dynamic LDS: the mode-1 pattern table)

The windowed regime: stencil view, near slots 0x3e, a halo, rare or 7 slots, MGCR_FUSED_TILE on, reach >= the threshold
(2^15).  PW only in the step apply; CARRY only in windowed forms, and in the 7-slot step apply PW wins over CARRY.  The
window is 2 x (1024 + 2 halo) x 16 bytes: 36 864 at halo 64, 49 152 at halo 256."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIN = " win=36864 lds=36864"
NOWIN = " win=0 lds=0"
ERR = "error=not the windowed form's case"
# stencil view below the threshold, dictionary and slab: the same form whoever launches (PW only where asked, never CARRY)
STORED = [
    ("sten-rare", "plain<4,9>", NOWIN),
    ("sten-7", "plain<3,7>", NOWIN),
    ("sten-9", "plain<3,9>", NOWIN),
    ("dict1-w7", "plain<1,7>", " win=0 lds=1400"),
    ("dict1-w5", "plain<1,0>", " win=0 lds=1400"),
    ("dict2-w7", "plain<2,7>", NOWIN),
    ("dict2-w27", "plain<2,0>", NOWIN),
    ("slab-w7", "plain<0,7>", NOWIN),
    ("slab-w8", "plain<0,0>", NOWIN),
]
EXPECTED = [
    "step tile-rare tile<9,1> pw=0 carry=0" + WIN,
    "step tile-rare-carried tile<9,1> pw=0 carry=1" + WIN,
    "step tile-rare-pw tile<9,1> pw=1 carry=0" + WIN,
    "step tile-rare-pw-carried tile<9,1> pw=1 carry=1" + WIN,
    "step tile-7 tile<7,0> pw=0 carry=0" + WIN,
    "step tile-7-carried tile<7,0> pw=0 carry=1" + WIN,
    # PW wins over CARRY: the same form with and without the carried flag (<7, false, PW, CARRY> does not exist)
    "step tile-7-pw tile<7,0> pw=1 carry=0" + WIN,
    "step tile-7-pw-carried tile<7,0> pw=1 carry=0" + WIN,
    "init tile-rare tile<9,1> pw=0 carry=0" + WIN,
    "init tile-rare-carried tile<9,1> pw=0 carry=1" + WIN,
    "init tile-7 tile<7,0> pw=0 carry=0" + WIN,
    "init tile-7-carried tile<7,0> pw=0 carry=1" + WIN,
    "init tile-7-carried-pw-asked tile<7,0> pw=0 carry=1" + WIN,
    "xr tile-rare " + ERR,
    "xr tile-rare-carried " + ERR,
    "xr tile-7 " + ERR,
    "xr tile-7-carried tile<7,0> pw=0 carry=1" + WIN,
    "xr tile-7-carried-ap-elsewhere " + ERR,
] + [
    "%s %s %s pw=0 carry=0%s" % (use, name, form, lds) for use in ("step", "xr", "init") for name, form, lds in STORED
] + [
    "step sten-rare-pw plain<4,9> pw=1 carry=0" + NOWIN,
    "step sten-7-pw-carried-asked plain<3,7> pw=1 carry=0" + NOWIN,
    "step dict1-w7-pw plain<1,7> pw=1 carry=0 win=0 lds=1400",
    "xr slab-w7-pw-asked plain<0,7> pw=0 carry=0" + NOWIN,
    # the regime's boundary: one row short of the threshold, on it, no halo, other near slots, nine common slots
    "step reach-below plain<3,7> pw=0 carry=0" + NOWIN,
    "step reach-equal tile<7,0> pw=0 carry=0" + WIN,
    "step halo-0 plain<3,7> pw=0 carry=0" + NOWIN,
    "step near-0x3c plain<3,7> pw=0 carry=0" + NOWIN,
    "step nine-common plain<3,9> pw=0 carry=0" + NOWIN,
    "step halo-256 tile<7,0> pw=0 carry=0 win=49152 lds=49152",
    # MGCR_FUSED_TILE=0 (nothing is carried outside the regime), MGCR_FUSED_TILE_REACH=1024
    "step tile-off plain<3,7> pw=0 carry=0" + NOWIN,
    "step tile-off-rare plain<4,9> pw=0 carry=0" + NOWIN,
    "xr tile-off plain<3,7> pw=0 carry=0" + NOWIN,
    "step min-reach-1024 tile<7,0> pw=0 carry=0" + WIN,
    "regime windowed 1 0 0",
    "regime xr-windowed 1 0 0",
    "xr xr-switch-off-launch tile<7,0> pw=0 carry=1" + WIN,
    "grid padded 1 63 64 72 512",
    "reach default 32768",
]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fused_form") / "fused_form_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "fused_form_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    return p.stdout.splitlines()


def test_every_case_printed_once(printed):
    assert [" ".join(l.split()[:2]) for l in printed] == [" ".join(l.split()[:2]) for l in EXPECTED]


@pytest.mark.parametrize("line", EXPECTED, ids=lambda l: "-".join(l.split()[:2]))
def test_form_selected(printed, line):
    key = line.split()[:2]
    got = [l for l in printed if l.split()[:2] == key]
    assert got == [line]
