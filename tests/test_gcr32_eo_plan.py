"""csrc/gcr32_eo_plan.h — the host plan of the low-precision GCR in even-odd form — against the numpy plan of
tests/gcr32_eo_cases.py, on the CPU.  tests/cpp/gcr32_eo_plan_check.cpp — a stand-alone program — is built with g++ and the address /
undefined-behaviour sanitizers and run on every case: the halves, their widths, slabs, tails and tile tables, the one real flag, the
float diagonals and c2 bit for bit, and the refusals with their messages."""
import os
import subprocess

import numpy as np
import pytest

from tests import evenodd_diag_cases as dc
from tests import gcr32_cases as g
from tests import gcr32_eo_cases as e
from tests.test_gcr32_plan import parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gcr32_eo_plan") / "gcr32_eo_plan_check")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mgpreconditionedgcr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "gcr32_eo_plan_check.cpp"), "-o", path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return path


def run(exe, tmp_path, c):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    k = complex(c.k) if c.k is not None else 0j
    with open(src, "wb") as f:
        np.array([c.n, c.col.size, g.TILE, c.parity is not None, c.form == "matrix"], np.int64).tofile(f)
        np.array([k.real, k.imag], np.float64).tofile(f)
        np.ascontiguousarray(c.rowptr, np.int64).tofile(f)
        np.ascontiguousarray(c.col, np.int64).tofile(f)
        np.ascontiguousarray(c.val, np.complex128).view(np.float64).tofile(f)
        if c.parity is not None:
            np.ascontiguousarray(c.parity, np.int8).tofile(f)
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    return p.stdout.splitlines(), dst


def read_plan(path, n):
    with open(path, "rb") as f:
        ne, no, diag, real, stored = (int(v) for v in np.fromfile(f, np.int64, 5))
        d = dict(ne=ne, no=no, has_diag=bool(diag), real=bool(real), stored=stored)
        d["parity"] = np.fromfile(f, np.int8, n)
        d["c2"] = np.fromfile(f, np.float32, 2)
        d["a_even"] = np.fromfile(f, np.float32, 2 * ne if diag else 0)
        d["inv_a_odd"] = np.fromfile(f, np.float32, 2 * no if diag else 0)
        nc = 1 if real else 2
        d["half"] = []
        for _ in range(2):
            W, npad, nt, tnnz, ntile = (int(v) for v in np.fromfile(f, np.int64, 5))
            h = dict(W=W, npad=npad)
            h["ell_col"] = np.fromfile(f, np.int32, W * npad).reshape(W, npad)
            h["ell_val"] = np.fromfile(f, np.float32, W * npad * nc).reshape(W, npad, nc)
            h["tail_rows"] = np.fromfile(f, np.int32, nt)
            h["tail_ptr"] = np.fromfile(f, np.int32, nt + 1)
            h["tail_col"] = np.fromfile(f, np.int32, tnnz)
            h["tail_val"] = np.fromfile(f, np.float32, tnnz * nc).reshape(tnnz, nc)
            h["tile_tail"] = np.fromfile(f, np.int32, ntile)
            d["half"].append(h)
        assert f.read() == b""
    return d


def floats(z):
    return np.ascontiguousarray(z, np.complex64).view(np.float32)


@pytest.mark.parametrize("name,k", e.all_cases())
def test_plan_equals_the_model(exe, tmp_path, name, k):
    c = e.case(name, k)
    p = e.plan_of(name)
    _, co = e.coefficients(c, p)
    out, dst = run(exe, tmp_path, c)
    assert out[0] == "OK %d %d %d %d" % (p.ne, p.no, int(p.has_diag), int(p.real)), out
    d = read_plan(dst, c.n)
    assert (d["ne"], d["no"], d["has_diag"], d["real"], d["stored"]) == (p.ne, p.no, p.has_diag, p.real, p.stored_bytes)
    assert np.array_equal(d["parity"], p.parity)
    assert np.array_equal(d["c2"].view(np.uint32), floats(np.array([co.c2])).view(np.uint32))
    if p.has_diag:
        assert np.array_equal(d["a_even"].view(np.uint32), floats(co.a_even).view(np.uint32))
        assert np.array_equal(d["inv_a_odd"].view(np.uint32), floats(co.inv_a_odd).view(np.uint32))
    for h, hp in zip(d["half"], p.hplans):
        assert (h["W"], h["npad"]) == (hp.W, hp.npad)
        assert np.array_equal(h["ell_col"], hp.ell_col)
        assert np.array_equal(h["ell_val"].view(np.uint32), parts(hp.ell_val, p.real).view(np.uint32))
        for key in ("tail_rows", "tail_ptr", "tail_col", "tile_tail"):
            assert np.array_equal(h[key], getattr(hp, key)), key
        assert np.array_equal(h["tail_val"].view(np.uint32), parts(hp.tail_val, p.real).view(np.uint32))


def test_the_cases_reach_what_they_are_there_for():
    """tails in both halves of the bipartite case, one of them behind the first tile; a real slab with c2 = 1; n_e != n_o; an odd n_e"""
    p = e.plan_of("bip_long")
    assert all(hp.tail_rows.size > 0 for hp in p.hplans) and any((hp.tail_rows >= g.TILE).any() for hp in p.hplans)
    assert all(int(np.diff(h.rowptr).max()) > hp.W for h, hp in zip(p.halves, p.hplans))
    b = e.plan_of("box_small")
    assert b.real and b.has_diag and (b.ne, b.no) == (158, 157)
    assert e.coefficients(e.case("box_small"), b)[1].c2 == 1
    t = e.plan_of("two_parts")
    assert t.ne != t.no and (np.diff(e.case("two_parts").rowptr) == 0).any()
    ch = e.plan_of("chain")
    assert (ch.ne, ch.no) == (23, 22) and not ch.has_diag
    s = e.plan_of("sample")
    assert (s.ne, s.no) == (1536, 1536) and not s.real
    assert e.plan_of("box_many").ne > 8 * g.TILE
    for name in ("d_open4d", "d_scalar", "sample_twisted"):
        assert e.plan_of(name).has_diag and not e.plan_of(name).real


@pytest.mark.parametrize("name", e.REJECTED)
def test_refusals_name_the_row(exe, tmp_path, name):
    c, row, word = e.rejected(name)
    assert e.refusal(c) == (row, word)
    out, _ = run(exe, tmp_path, c)
    assert out[0] == "INVALID" and ("row %d" % row) in out[1] and word in out[1], out


def test_a_conflicting_entry_is_named_as_the_fp64_plan_names_it(exe, tmp_path):
    d, (r, cc) = dc.rejected("triangle")
    out, _ = run(exe, tmp_path, e.ECase(d.name, "dirac", d.k, d.n, d.rowptr, d.col, d.val, None))
    assert out[0] == "INVALID" and ("entry (row %d, column %d)" % (r, cc)) in out[1], out


def test_a_k_whose_square_overflows_float_is_refused(exe, tmp_path):
    out, _ = run(exe, tmp_path, e.case("chain", 1e30))
    assert out[0] == "INVALID" and "c^2" in out[1] and "single precision" in out[1], out


def test_an_empty_matrix(exe, tmp_path):
    c = e.ECase("empty", "dirac", 0.1, 0, np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.complex128), None)
    out, _ = run(exe, tmp_path, c)
    assert out[0] == "OK 0 0 0 1", out
    c = e.ECase("rows_only", "matrix", None, 3, np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0, np.complex128), None)
    out, _ = run(exe, tmp_path, c)                   # matrix form with d = 0 everywhere, all rows even: nothing odd to invert
    assert out[0] == "OK 3 0 1 1", out
