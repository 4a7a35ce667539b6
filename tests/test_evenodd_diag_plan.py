"""The host plan of a matrix with a site diagonal (csrc/evenodd_plan.h, evenodd_plan_build_diag) on the CPU:
tests/cpp/evenodd_diag_plan_check.cpp — a stand-alone program — is built with g++ and the address / undefined-behaviour sanitizers
and run as a child process on the cases of tests/evenodd_diag_cases.py; the diagonal d (stored entries added in stored order), the
parity, the index lists and both off-diagonal half matrices are compared with the numpy model, and the refusals must name the entry
the model names.  evenodd_plan_build itself must go on refusing a diagonal entry."""
import os
import subprocess

import numpy as np
import pytest

from tests import evenodd_cases as ec
from tests import evenodd_diag_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("d_sample", "d_open4d", "d_chain", "d_two_parts", "d_scalar", "d_w7_slab", "poisson_box", "sample_m", "sample_twisted", "dup_diag",
         "chain_zero_even")     # (the 2^16-row cases have the halves of hopping cases tests/test_evenodd_plan.py already runs)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("evenodd_diag_plan") / "evenodd_diag_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "evenodd_diag_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return path


def run(exe, tmp_path, c, parity=None):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([c.n, c.col.size, 0 if parity is None else 1], np.int64).tofile(f)
        c.rowptr.astype(np.int64).tofile(f)
        c.col.astype(np.int64).tofile(f)
        np.ascontiguousarray(c.val, np.complex128).view(np.float64).tofile(f)
        if parity is not None:
            np.asarray(parity, np.int64).tofile(f)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    return p.stdout.splitlines(), dst


def read_plan(path, n):
    with open(path, "rb") as f:
        ne, no, nnz_eo, nnz_oe = np.fromfile(f, np.int64, 4)
        out = dict(parity=np.fromfile(f, np.int64, n), even=np.fromfile(f, np.int64, ne), odd=np.fromfile(f, np.int64, no),
                   index=np.fromfile(f, np.int64, n))
        for name, nrow, nnz in (("eo", ne, nnz_eo), ("oe", no, nnz_oe)):
            out[name] = (np.fromfile(f, np.int64, nrow + 1), np.fromfile(f, np.int64, nnz), np.fromfile(f, np.float64, 2 * nnz).view(np.complex128))
        out["d"] = np.fromfile(f, np.float64, 2 * n).view(np.complex128)
        assert f.read() == b""
    return out


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


@pytest.mark.parametrize("name", CASES)
def test_plan_equals_the_model(exe, tmp_path, name):
    c, m = dc.case(name), dc.case_plan(name)
    _, d, n_diag = dc.strip(name)
    lines, dst = run(exe, tmp_path, c)
    assert lines[0] == "OK %d %d %d" % (m.even.size, m.odd.size, n_diag)
    got = read_plan(dst, c.n)
    assert np.array_equal(bits(got["d"]), bits(d))                  # added in stored order: bit for bit
    assert np.array_equal(got["parity"], m.parity) and np.array_equal(got["even"], m.even) and np.array_equal(got["odd"], m.odd)
    assert np.array_equal(got["index"], m.index)
    for key, half in (("eo", m.eo), ("oe", m.oe)):
        rowptr, col, val = got[key]
        assert np.array_equal(rowptr, half[2]) and np.array_equal(col, half[3]) and np.array_equal(val, half[4]), key   # off-diagonal only


def test_a_matrix_without_a_diagonal_gives_the_plain_plan(exe, tmp_path):
    c, m = ec.case("open4d"), ec.case_plan("open4d")
    lines, dst = run(exe, tmp_path, c)
    assert lines[0] == "OK %d %d 0" % (m.even.size, m.odd.size)
    got = read_plan(dst, c.n)
    assert not got["d"].any() and np.array_equal(got["parity"], m.parity) and np.array_equal(got["eo"][2], m.eo[4])


def test_a_given_parity_is_taken_and_checked(exe, tmp_path):
    c = dc.case("sample_twisted")
    lines, dst = run(exe, tmp_path, c, 1 - ec.sample_site_parity())
    assert lines[0] == "OK 1536 1536 3072" and np.array_equal(read_plan(dst, c.n)["even"], ec.case_plan("sample").odd)
    # a wrong caller bit is refused with the off-diagonal entry named, exactly as without a diagonal
    hop, par, (row, col) = ec.rejected("flipped")
    lines, _ = run(exe, tmp_path, dc.DCase("flipped", "dirac", 0.1, hop.n, *dc.with_diagonal(hop, np.arange(hop.n), np.ones(hop.n))), par)
    assert lines[0] == "INVALID %d %d" % (row, col) and "row %d, column %d" % (row, col) in lines[1]


def test_an_odd_cycle_is_still_refused(exe, tmp_path):
    c, (row, col) = dc.rejected("triangle")
    lines, _ = run(exe, tmp_path, c)
    assert lines[0] == "INVALID %d %d" % (row, col)
    assert "row %d, column %d" % (row, col) in lines[1] and "pure hopping matrix" in lines[1]


def test_the_plain_plan_goes_on_refusing_a_diagonal(tmp_path_factory, tmp_path):
    path = str(tmp_path_factory.mktemp("evenodd_plain_plan") / "evenodd_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "evenodd_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    lines, _ = run(path, tmp_path, dc.case("dup_diag"))
    assert lines[0] == "INVALID 3 3" and "a diagonal entry" in lines[1]
