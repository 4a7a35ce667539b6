"""The host plan of a matrix with a dense block per site (csrc/evenodd_plan.h, evenodd_plan_build_block) on the CPU:
tests/cpp/evenodd_block_plan_check.cpp — a stand-alone program — is built with g++ and the address / undefined-behaviour sanitizers
and run as a child process on the cases of tests/evenodd_block_cases.py; the blocks of stored values (entries of one position added
in stored order), the site colouring expanded to the row parity, the index lists and both inter-site half matrices are compared
with the numpy model, and every refusal must name what the model names."""
import os
import subprocess

import numpy as np
import pytest

from tests import evenodd_cases as ec
from tests import evenodd_block_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tuple(n for n in bc.ALL if n != "grid2d_varied_b3")      # (its halves are those of a hopping case tests/test_evenodd_plan.py runs)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("evenodd_block_plan") / "evenodd_block_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "evenodd_block_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return path


def run(exe, tmp_path, c, parity=None):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        np.array([c.n, c.col.size, 0 if parity is None else 1, c.bs], np.int64).tofile(f)
        c.rowptr.astype(np.int64).tofile(f)
        c.col.astype(np.int64).tofile(f)
        np.ascontiguousarray(c.val, np.complex128).view(np.float64).tofile(f)
        if parity is not None:
            np.asarray(parity, np.int64).tofile(f)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr[-4000:]   # sanitizer reports go to stderr
    return p.stdout.splitlines(), dst


def read_plan(path, n, bs):
    with open(path, "rb") as f:
        ne, no, nnz_eo, nnz_oe = np.fromfile(f, np.int64, 4)
        out = dict(parity=np.fromfile(f, np.int64, n), even=np.fromfile(f, np.int64, ne), odd=np.fromfile(f, np.int64, no),
                   index=np.fromfile(f, np.int64, n))
        for name, nrow, nnz in (("eo", ne, nnz_eo), ("oe", no, nnz_oe)):
            out[name] = (np.fromfile(f, np.int64, nrow + 1), np.fromfile(f, np.int64, nnz), np.fromfile(f, np.float64, 2 * nnz).view(np.complex128))
        out["be"] = np.fromfile(f, np.float64, 2 * ne * bs).view(np.complex128).reshape(ne // bs, bs, bs)
        out["bo"] = np.fromfile(f, np.float64, 2 * no * bs).view(np.complex128).reshape(no // bs, bs, bs)
        assert f.read() == b""
    return out


def bits(z):
    return np.ascontiguousarray(z, np.complex128).view(np.uint64)


def compare(got, m, d, bs):
    se, so = bc.site_lists(m, bs)
    assert np.array_equal(bits(got["be"]), bits(d[se])) and np.array_equal(bits(got["bo"]), bits(d[so]))   # added in stored order
    assert np.array_equal(got["parity"], m.parity) and np.array_equal(got["even"], m.even) and np.array_equal(got["odd"], m.odd)
    assert np.array_equal(got["index"], m.index)
    for key, half in (("eo", m.eo), ("oe", m.oe)):
        rowptr, col, val = got[key]
        assert np.array_equal(rowptr, half[2]) and np.array_equal(col, half[3]) and np.array_equal(val, half[4]), key   # inter-site only


@pytest.mark.parametrize("name", CASES)
def test_plan_equals_the_model(exe, tmp_path, name):
    c, m = bc.case(name), bc.case_plan(name)
    _, d, n_in = bc.strip(name)
    lines, dst = run(exe, tmp_path, c)
    assert lines[0] == "OK %d %d %d" % (m.even.size, m.odd.size, n_in)
    compare(read_plan(dst, c.n, c.bs), m, d, c.bs)
    assert (np.diff(m.even.reshape(-1, c.bs), axis=1) == 1).all() and (m.even[::c.bs] % c.bs == 0).all()   # a site's rows stay together


def test_a_given_parity_is_taken(exe, tmp_path):
    c = bc.case("sample_h05")
    par = 1 - ec.sample_site_parity()
    lines, dst = run(exe, tmp_path, c, par)
    assert lines[0].startswith("OK 1536 1536 ")
    compare(read_plan(dst, c.n, c.bs), bc.plan_of(c, par), bc.strip("sample_h05")[1], c.bs)


def test_block_size_and_row_count_are_checked(exe, tmp_path):
    for name, word in (("bs0", "bs = 0"), ("bs17", "bs = 17"), ("not_whole", "n = 15")):
        lines, _ = run(exe, tmp_path, bc.rejected(name))
        assert lines[0] == "INVALID -1 -1" and word in lines[1], lines


def test_an_odd_cycle_of_sites_names_an_inter_site_entry(exe, tmp_path):
    c, (row, col) = bc.rejected("triangle")
    lines, _ = run(exe, tmp_path, c)
    assert lines[0] == "INVALID %d %d" % (row, col) and "row %d, column %d" % (row, col) in lines[1]


def test_a_parity_that_splits_a_site_names_the_row(exe, tmp_path):
    c, par, row, site = bc.rejected("split_parity")
    lines, _ = run(exe, tmp_path, c, par)
    assert lines[0] == "INVALID -1 -1" and "parity[%d]" % row in lines[1] and "site %d" % site in lines[1], lines


def test_a_parity_that_joins_two_sites_of_one_colour_names_the_entry(exe, tmp_path):
    c, par, (row, col) = bc.rejected("flipped")
    lines, _ = run(exe, tmp_path, c, par)
    assert lines[0] == "INVALID %d %d" % (row, col) and "row %d, column %d" % (row, col) in lines[1]
